// Shared pieces of the index scan kernels (bf16: index_topk.hip, index_filter.hip; fp8:
// index_fp8.hip, index_filter_fp8.hip).
#pragma once
#include "common.h"

namespace symb {

// counted vector-memory wait (loads, LDS-DMA and stores retire in issue order)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

template <int AUX>
__device__ __forceinline__ void glds16_aux(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, AUX);
}

// compile-time loop: f(integral_constant<int, i>) for i = I .. N - 1
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    static_for<I + 1, N>(f);
  }
}

// no-op DMA functor for MFMA chains that issue no LDS-DMA pieces
struct NoDma {
  __device__ __forceinline__ void operator()(int) const {}
};

// ---- masked scans (index_filter.hip, index_filter_fp8.hip): mask words, hand-issued scalar loads
// mask word of 64-row tile `tile` with the bits of rows at or past n_valid cleared
__device__ __forceinline__ uint64_t live_word(uint64_t w, int tile, int n_valid) {
  const long rem = (long)n_valid - (long)tile * 64;
  if (rem < 64) w = rem > 0 ? (w & ((1ull << rem) - 1)) : 0ull;
  return w;
}

// Tile indices and mask words are wave-uniform, so they are read by scalar loads, issued by hand
// and waited for by hand (swait): a compiler-placed scalar load would be waited for with
// lgkmcnt(0) wherever its value is first used, in the middle of a counted ds_read pipeline.
__device__ __forceinline__ void sload_i32(int& dst, const int* p) {
  asm volatile("s_load_dword %0, %1, 0x0" : "=s"(dst) : "s"(p));
}
__device__ __forceinline__ void sload_u64(uint64_t& dst, const uint64_t* p) {
  asm volatile("s_load_dwordx2 %0, %1, 0x0" : "=s"(dst) : "s"(p));
}
// every scalar load (and ds_read) of this wave has landed; the asm names the loaded values so no
// use of them can be scheduled above the wait
__device__ __forceinline__ void swait(int& a, int& b, uint64_t& w) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a), "+s"(b), "+s"(w)::"memory");
}

// the same wait for N loaded ints (volatile asm statements keep their order, so each value is
// re-defined below the wait)
template <int N>
__device__ __forceinline__ void swait_n(int (&v)[N]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+s"(v[i]));
}

template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&tv)[KMAX], int (&ti)[KMAX], float s, int id) {
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    const bool sw = s > tv[i];
    const float ov = tv[i];
    const int oi = ti[i];
    tv[i] = sw ? s : ov;
    ti[i] = sw ? id : oi;
    s = sw ? ov : s;
    id = sw ? oi : id;
  }
}

// Wave-wide max of a float, valid in lane 63: DPP row shifts fold each 16-lane row, then two row
// broadcasts fold the rows (max is idempotent, so lanes whose DPP source is out of range simply
// keep their own value).
__device__ __forceinline__ float wave_max63(float v) {
  int x = __float_as_int(v);
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x111, 0xf, 0xf, false))));
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x112, 0xf, 0xf, false))));
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x114, 0xf, 0xf, false))));
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x118, 0xf, 0xf, false))));
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x142, 0xa, 0xf, false))));
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x143, 0xc, 0xf, false))));
  return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}

// KMAX rounds of a wave-wide "pop the best head": every lane holds a descending list of L
// candidates; each round the wave max of the heads (DPP, no LDS), the lowest lane holding it gives
// up its head (its list shifts by one) and lane r keeps round r's winner.  Replaces the LDS tree
// of pairwise merges (8 rounds x 2 barriers x a 16-step serial merge per level).
template <int KMAX, int L>
__device__ __forceinline__ void wave_pop_topk(float (&tv)[L], int (&ti)[L], int lane, float& rv,
                                              int& ri) {
  rv = -INFINITY;
  ri = -1;
#pragma unroll
  for (int r = 0; r < KMAX; ++r) {
    const float mx = wave_max63(tv[0]);
    const uint64_t hit = __ballot(tv[0] == mx);
    const int win = hit ? (int)__builtin_ctzll(hit) : 0;
    const int id = __builtin_amdgcn_readlane(ti[0], win);
    if (lane == r) {
      rv = mx;
      ri = id;
    }
    if (lane == win) {
#pragma unroll
      for (int i = 0; i + 1 < L; ++i) {
        tv[i] = tv[i + 1];
        ti[i] = ti[i + 1];
      }
      tv[L - 1] = -INFINITY;
      ti[L - 1] = -1;
    }
  }
}

// Same result as topk_insert but with no serial chain: every slot decides from the ORIGINAL
// sorted list (monotone "s > tv[i]" flags), so the 16 compare/select pairs issue back to back.
template <int KMAX>
__device__ __forceinline__ void topk_insert_par(float (&tv)[KMAX], int (&ti)[KMAX], float s, int id) {
  float nv[KMAX];
  int ni[KMAX];
  nv[0] = s > tv[0] ? s : tv[0];
  ni[0] = s > tv[0] ? id : ti[0];
#pragma unroll
  for (int i = 1; i < KMAX; ++i) {
    const float shv = s > tv[i - 1] ? tv[i - 1] : s;   // value slot i takes if s beats it
    const int shi = s > tv[i - 1] ? ti[i - 1] : id;
    nv[i] = s > tv[i] ? shv : tv[i];
    ni[i] = s > tv[i] ? shi : ti[i];
  }
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    tv[i] = nv[i];
    ti[i] = ni[i];
  }
}

constexpr int TOPK_WAVES = 8;

// ---- hand-counted LDS fragment pipeline -------------------------------------------------------
// hipcc will not count ds_reads around the DMA ring (it drains lgkmcnt(0) before every few MFMAs),
// so the A fragments are read by inline asm and each MFMA waits with a counted lgkmcnt(N) whose
// asm names the fragment as "+v" (the MFMA depends on it and cannot be hoisted above the wait).
template <int OFF>
__device__ __forceinline__ void ds_read16(bf16x8& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
template <int N>
__device__ __forceinline__ void lgkm_wait(bf16x8& v) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "i"(N));
}

// Fragment ks lives at  base + voff[ks % M] + (ks / M) * 256  (the XOR swizzle only touches the
// low 4 bits of the 16-byte chunk index, so the per-lane part repeats every M k-steps).
// DMA (functor, may be a no-op): DMA(i) issues LDS-DMA piece i of the next tile; pieces are
// spread one per DMA_EVERY MFMAs so the waves' DMA issue interleaves with their matrix work.
template <int KS, int NKS, int PF, int M, bool M32, int DMA_EVERY = 0, int DMA_PIECES = 0>
struct FragChain {
  static constexpr int R = PF + 1;  // ring slots: a slot is refilled one MFMA after its last use
  template <class Acc, class Dma = NoDma>
  __device__ __forceinline__ static void run(Acc& acc, bf16x8 (&a)[R], const bf16x8 (&qf)[NKS],
                                             const uint32_t (&voff)[M], uint32_t base,
                                             const Dma& dma = Dma()) {
    if constexpr (DMA_EVERY > 0 && KS % DMA_EVERY == 0 && KS / DMA_EVERY < DMA_PIECES)
      dma(KS / DMA_EVERY);
    constexpr int outstanding = (NKS - KS < PF) ? (NKS - KS) : PF;
    lgkm_wait<outstanding - 1>(a[KS % R]);
    if constexpr (M32)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[KS % R], qf[KS], acc, 0, 0, 0);
    else
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[KS % R], qf[KS], acc, 0, 0, 0);
    if constexpr (KS + PF < NKS)
      ds_read16<((KS + PF) / M) * 256>(a[(KS + PF) % R], base + voff[(KS + PF) % M]);
    if constexpr (KS + 1 < NKS)
      FragChain<KS + 1, NKS, PF, M, M32, DMA_EVERY, DMA_PIECES>::run(acc, a, qf, voff, base, dma);
  }
};

template <int J, int PF, int M, int R>
__device__ __forceinline__ void frag_prologue(bf16x8 (&a)[R], const uint32_t (&voff)[M],
                                              uint32_t base) {
  ds_read16<(J / M) * 256>(a[J % R], base + voff[J % M]);
  if constexpr (J + 1 < PF) frag_prologue<J + 1, PF, M, R>(a, voff, base);
}

// ---- pieces the register-list scans share ------------------------------------------------------
// (bf16: index_scan_topk_kernel and its masked form index_scan_filter_kernel; acc_reg_row also
// the masked fp8 scan.)  M32: 32x32 MFMA tiles (bf16 at D = 384, fp8), else 16x16.  Only what
// leaves every instantiation's instruction stream as it was is shared: the other setup pieces are
// textually equal within a pair, but as helpers each of them rescheduled the kernels' prologues
// (profiles/retire_scan_diag/README.md has the list).

// Row, within its sub-tile, of accumulator register r of a lane, less the lane's own
// 4 * (lane >> 5) (32x32: four rows of every eight) or 4 * (lane >> 4) (16x16: four in a row).
template <bool M32>
__device__ __forceinline__ constexpr int acc_reg_row(int r) {
  return M32 ? (r & 3) + 8 * (r >> 2) : r;
}

// The query's B fragments: k-step ks of a lane is 8 consecutive k of Q[query] (qp).
template <int D, bool M32, int NKS>
__device__ __forceinline__ void load_query_frags(bf16x8 (&qf)[NKS], const __bf16* qp, int lane) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int k0 = M32 ? ks * 16 + (lane >> 5) * 8 : ks * 32 + (lane >> 4) * 8;
    qf[ks] = *reinterpret_cast<const bf16x8*>(qp + k0);
  }
}

}  // namespace symb
