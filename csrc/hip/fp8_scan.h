// Pieces shared by the fp8 (OCP e4m3) index scans: index_fp8.hip (every row) and
// index_filter_fp8.hip (the rows a mask allows).  See index_fp8.hip's header for the design.
#pragma once
#include "scan_common.h"

namespace symb {

typedef __attribute__((ext_vector_type(8))) int i32x8;  // fp8 MFMA operand: 32 bytes per lane
typedef __attribute__((ext_vector_type(4))) int i32x4;

template <int OFF>
__device__ __forceinline__ void ds_read16_i(i32x4& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
template <int N>
__device__ __forceinline__ void lgkm_wait2(i32x4& a, i32x4& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "i"(N));
}

// LDS image swizzle: within each group of G 16-byte chunks of a row, chunk c is stored at
// c ^ f(row).  G = 16, f = row & 15 for rows of 512 / 768 / 1024 bytes (a multiple of 256 B);
// D = 384 (24 chunks, rows 96 dwords ~ 32 mod 64 banks) uses G = 8, f = (row >> 1) & 7, which
// keeps every 16-lane ds_read_b128 group of a 32-row fragment conflict-free (rows 2i and 2i+1
// sit in opposite 128-byte halves of the bank row, and f separates the pairs).
template <int D> struct Fp8Swz {
  static constexpr int G = D % 256 == 0 ? 16 : 8;
  __device__ __forceinline__ static int f(int row) { return G == 16 ? (row & 15) : ((row >> 1) & 7); }
  __device__ __forceinline__ static int phys(int c, int row) { return (c & ~(G - 1)) | ((c & (G - 1)) ^ f(row)); }
};

// fragment ks of a sub-tile: row r = lane & 31 holds bytes [64 ks + 32 h, +32), h = lane >> 5,
// i.e. 16-byte chunks c = 4 ks + 2 h + j (j = 0, 1), stored at Fp8Swz::phys(c, r): the per-lane
// part repeats every P = G / 4 k-steps (voff[ks % P][j]) and the rest is the immediate
// (ks / P) * 16 G bytes.
template <int J, int PF, int R, int G>
__device__ __forceinline__ void fp8_prologue(i32x4 (&lo)[R], i32x4 (&hi)[R],
                                             const uint32_t (&voff)[8], uint32_t base) {
  constexpr int P = G / 4;
  ds_read16_i<(J / P) * 16 * G>(lo[J % R], base + voff[(J % P) * 2]);
  ds_read16_i<(J / P) * 16 * G>(hi[J % R], base + voff[(J % P) * 2 + 1]);
  if constexpr (J + 1 < PF) fp8_prologue<J + 1, PF, R, G>(lo, hi, voff, base);
}

template <int KS, int NKS, int PF, int DMA_PIECES, int G>
struct Fp8Chain {
  static constexpr int R = PF + 1;
  template <class Dma>
  __device__ __forceinline__ static void run(f32x16& acc0, f32x16& acc1, i32x4 (&lo)[R],
                                             i32x4 (&hi)[R], const i32x8 (&q0)[NKS],
                                             const i32x8 (&q1)[NKS], const uint32_t (&voff)[8],
                                             uint32_t base, const Dma& dma) {
    if constexpr (KS < DMA_PIECES) dma(KS);
    constexpr int in_flight = (NKS - KS < PF) ? (NKS - KS) : PF;  // fragments incl. this one
    lgkm_wait2<2 * (in_flight - 1)>(lo[KS % R], hi[KS % R]);
    const i32x8 a = __builtin_shufflevector(lo[KS % R], hi[KS % R], 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (KS == 0) {
      asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, 0" : "=&v"(acc0) : "v"(a), "a"(q0[0]));
      asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, 0" : "=&v"(acc1) : "v"(a), "a"(q1[0]));
    } else {
      asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0" : "+v"(acc0) : "v"(a), "a"(q0[KS]));
      asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0" : "+v"(acc1) : "v"(a), "a"(q1[KS]));
    }
    if constexpr (KS + 1 == NKS)  // XDL write -> VALU read of the accumulators (16-pass: 19 states)
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
    if constexpr (KS + PF < NKS) {
      constexpr int J = KS + PF, P = G / 4;
      ds_read16_i<(J / P) * 16 * G>(lo[J % R], base + voff[(J % P) * 2]);
      ds_read16_i<(J / P) * 16 * G>(hi[J % R], base + voff[(J % P) * 2 + 1]);
    }
    if constexpr (KS + 1 < NKS)
      Fp8Chain<KS + 1, NKS, PF, DMA_PIECES, G>::run(acc0, acc1, lo, hi, q0, q1, voff, base, dma);
  }
};

// Ring geometry per D: SUBS sub-tiles of 32 rows per barrier, NS tiles in the LDS ring.
// (symb_filter_fp8_ring_depth reports NS to the tests, which bracket it with slice lengths.)
template <int D> struct Fp8Cfg;
template <> struct Fp8Cfg<1024> { static constexpr int SUBS = 2, NS = 2; };  // 2 x 64 KiB
template <> struct Fp8Cfg<768> { static constexpr int SUBS = 1, NS = 6; };   // 6 x 24 KiB
template <> struct Fp8Cfg<512> { static constexpr int SUBS = 2, NS = 4; };   // 4 x 32 KiB
template <> struct Fp8Cfg<384> { static constexpr int SUBS = 2, NS = 5; };   // 5 x 24 KiB
template <> struct Fp8Cfg<256> { static constexpr int SUBS = 2, NS = 6; };   // 6 x 16 KiB

}  // namespace symb
