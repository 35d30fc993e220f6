// The per-query mask words of the masked scans' GROUPED forms (bf16: filter_scan.h; fp8:
// fp8_filter_scan.h, fp8_emit.h): mask8 is uint64 [n_words][MASK_GROUPS], 64 bytes per 64-row tile,
// slot g = the mask word of group g.  The eight words of a tile are wave-uniform and come by one
// hand-issued scalar load (as sload_u64, scan_common.h); a lane then picks its group's word.
#pragma once
#include "scan_common.h"

namespace symb {

constexpr int MASK_GROUPS = 8;

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

// the eight mask words of one tile, one hand-issued scalar load (as sload_u64, scan_common.h)
__device__ __forceinline__ void sload_mask8(u32x16& dst, const uint64_t* p) {
  asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(dst) : "s"(p));
}
// swait (scan_common.h) with the eight words in place of the one
__device__ __forceinline__ void swait_mask8(int& a, int& b, u32x16& w) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a), "+s"(b), "+s"(w)::"memory");
}
// the word of group grp (0 .. 7, per lane) out of the eight wave-uniform ones.  SEQ: each
// compare is tied to its two selects, so one compare mask is live at a time; left to itself the
// scheduler runs the seven compares first and holds seven mask pairs (the fp8 scan, whose SGPR
// file is full, spills them).
template <bool SEQ = false>
__device__ __forceinline__ uint64_t pick_word(const u32x16& w, int grp) {
  uint32_t lo = w[0], hi = w[1];
#pragma unroll
  for (int g = 1; g < MASK_GROUPS; ++g) {
    lo = grp == g ? w[2 * g] : lo;
    hi = grp == g ? w[2 * g + 1] : hi;
    if constexpr (SEQ) asm volatile("" : "+v"(lo), "+v"(hi), "+v"(grp));
  }
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace symb
