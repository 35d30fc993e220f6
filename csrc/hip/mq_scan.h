// Pieces the emitting bf16 scans share (index_mq.hip: index_scan_mq_kernel; index_mq_filter.hip:
// its masked form index_scan_mq_filter_kernel): the per-width geometry, the hand-issued MFMA and
// its counted A-fragment pipeline.  index_mq.hip's header has the design.
#pragma once
#include "scan_common.h"

namespace symb {

namespace mq {
constexpr int WAVES = 8;
constexpr int SUB = 16;                     // rows per MFMA chain
constexpr int PIECE = 1024;                 // LDS bytes per (sub-tile, k-step) piece
constexpr int PF = 3;                       // fragment reads in flight
constexpr int R = PF + 1;                   // fragment ring slots
// per-wave candidate stage in LDS after the ring: score f32, row i32, query-in-wave u16
constexpr int STW = 192;                    // staged candidates per wave (flushed past STW - 64)
constexpr int STAGE_BYTES = STW * 10;
}  // namespace mq

// Geometry per row width.  Queries stay resident as B fragments: SETS x D/32 k-steps x 4 VGPRs,
// at most 192 of a wave's 256 registers, so the query sets per wave shrink as D grows --
//   D = 384 : 64-row tiles (48 KiB), 3-deep ring, up to 4 sets (512 queries per workgroup);
//   D = 768 : 32-row tiles (48 KiB), 3-deep ring, 2 sets (256 queries: the reference's 768-d
//             collection, vector_memory_service/src/main.rs:22);
//   D = 1024: 16-row tiles (32 KiB), 4-deep ring, 1 set (128 queries).
template <int D> struct MqGeo {
  static constexpr int NKS = D / 32;                    // 16x16x32 k-steps over D
  static constexpr int TR = D == 384 ? 64 : D == 768 ? 32 : 16;   // rows per barrier interval
  static constexpr int NSUB = TR / mq::SUB;
  static constexpr int NS = D == 1024 ? 4 : 3;          // LDS ring depth in tiles
  static constexpr int TILE_BYTES = TR * D * 2;
  static constexpr int LOADS = TILE_BYTES / (1024 * mq::WAVES);  // LDS-DMA pieces per wave per tile
  static constexpr int DMA_EVERY = NKS / LOADS;         // k-steps between DMA pieces in sub-tile 0
  static constexpr int MAX_SETS = D == 384 ? 4 : D == 768 ? 2 : 1;
  static constexpr int LDS_BYTES = NS * TILE_BYTES + mq::WAVES * mq::STAGE_BYTES;
  static_assert(D == 384 || D == 768 || D == 1024, "row width");
  static_assert(TILE_BYTES % (1024 * mq::WAVES) == 0, "tile must split evenly over waves");
  static_assert(NSUB * NKS * mq::PIECE == TILE_BYTES, "a tile is NSUB x NKS pieces");
  static_assert(LOADS * DMA_EVERY <= NKS && DMA_EVERY >= 1, "DMA pieces must fit the first chain");
  static_assert(LDS_BYTES <= 160 * 1024, "ring + stages exceed the CU's 160 KiB");
  static_assert(NKS % mq::R == 0, "cross-chain prefetch: fragment j of the next chain must use slot j % R");
};

template <int OFF>
__device__ __forceinline__ void mq_read16(bf16x8& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
template <int N>
__device__ __forceinline__ void mq_lgkm(bf16x8& v) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "i"(N));
}

// One 16x16x32 MFMA per query set.  Hand-issued so the 192 query registers stay put as the B
// operand (VGPRs: naming them as AGPRs makes the compiler split the 256-register budget 128/128
// and shuttle queries between the files).
template <bool FIRST>
__device__ __forceinline__ void mq_mfma(f32x4& acc, const bf16x8& a, const bf16x8& q) {
  if constexpr (FIRST)
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(q));
  else
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(q));
}

// k-step KS of one 16-row sub-tile: wait for its A fragment, 4 MFMAs (one per query set), then
// refill the ring slot PF steps ahead -- in the last PF steps with the first fragments of the
// NEXT sub-tile (at ``next``, when NEXT), so its chain starts without an LDS round trip.
// DMA(i) issues LDS-DMA piece i of a later tile.
template <int D, int KS, int DMA_PIECES, bool NEXT, int SETS>
struct MqChain {
  static constexpr int NKS = MqGeo<D>::NKS, DMA_EVERY = MqGeo<D>::DMA_EVERY;
  template <class Dma>
  __device__ __forceinline__ static void run(f32x4 (&acc)[SETS], bf16x8 (&a)[mq::R],
                                             const bf16x8 (&qf)[SETS][NKS],
                                             uint32_t base, uint32_t next, const Dma& dma) {
    using namespace mq;
    if constexpr (DMA_PIECES > 0 && KS % DMA_EVERY == 0 && KS / DMA_EVERY < DMA_PIECES)
      dma(KS / DMA_EVERY);
    constexpr int outstanding = (NEXT || NKS - KS >= PF) ? PF : (NKS - KS);
    mq_lgkm<outstanding - 1>(a[KS % R]);
#pragma unroll
    for (int s = 0; s < SETS; ++s) mq_mfma<KS == 0>(acc[s], a[KS % R], qf[s][KS]);
    // XDL result -> VALU read (the emission test reads acc right after the chain): the compiler
    // pads nothing inside asm, so cover the MFMA's result latency here.
    if constexpr (KS + 1 == NKS) asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    // base / next: this lane's fragment address in piece 0 of this / the next sub-tile
    if constexpr (KS + PF < NKS)
      mq_read16<(KS + PF) * PIECE>(a[(KS + PF) % R], base);
    else if constexpr (NEXT)  // fragment KS + PF - NKS of the next sub-tile, same ring slot order
      mq_read16<(KS + PF - NKS) * PIECE>(a[(KS + PF) % R], next);
    if constexpr (KS + 1 < NKS)
      MqChain<D, KS + 1, DMA_PIECES, NEXT, SETS>::run(acc, a, qf, base, next, dma);
  }
};

// A pointer the compiler must treat as wave-uniform (SGPR pair): with it the LDS-DMA issues in the
// SGPR-base + 32-bit VGPR-offset form instead of a per-piece 64-bit VGPR address.
__device__ __forceinline__ const char* mq_uniform(const char* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

template <int J>
__device__ __forceinline__ void mq_prologue(bf16x8 (&a)[mq::R], uint32_t base) {
  mq_read16<J * mq::PIECE>(a[J % mq::R], base);
  if constexpr (J + 1 < mq::PF) mq_prologue<J + 1>(a, base);
}

}  // namespace symb
