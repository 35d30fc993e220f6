// Pieces the emitting e4m3 scans share (index_emit_fp8.hip: index_scan_emit_fp8_kernel;
// index_emit_group_fp8.hip: its form under a mask per query): the max over a lane's accumulators
// and the gated zeroing of the candidate counters.
#pragma once
#include "fp8_scan.h"
#include "mq_scan.h"

namespace symb {

// max of a lane's 16 accumulators by v_max3 (fmaxf would add NaN-canonicalising maxes)
__device__ __forceinline__ float fp8_max16(const f32x16& a) {
  float m;
  asm volatile(
      "v_max3_f32 %0, %1, %2, %3\n\t"
      "v_max3_f32 %0, %0, %4, %5\n\t"
      "v_max3_f32 %0, %0, %6, %7\n\t"
      "v_max3_f32 %0, %0, %8, %9\n\t"
      "v_max3_f32 %0, %0, %10, %11\n\t"
      "v_max3_f32 %0, %0, %12, %13\n\t"
      "v_max3_f32 %0, %0, %14, %15\n\t"
      "v_max3_f32 %0, %0, %16, %16"
      : "=&v"(m)
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]),
        "v"(a[8]), "v"(a[9]), "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]),
        "v"(a[15]));
  return m;
}

// cand_n[0 .. NQ) = 0 on stream st, under the scan's gate when there is one: with *gate == 0
// the counters keep what they held.  The kernel behind it is defined once, in
// index_emit_fp8.hip (each .hip is its own translation unit; both scans call this).
int emit_fp8_zero_counts(int* cand_n, int NQ, const int* gate, hipStream_t st);

}  // namespace symb
