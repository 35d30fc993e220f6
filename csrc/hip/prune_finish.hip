// The pruned search's finish in one launch: the exact bf16 re-score of every candidate
// (rescore_bf16_kernel, index_i8.hip) and the top-k of the re-scored list
// (topk_select_counted_kernel, index_mq.hip), one workgroup per query.
//
// Why (profiles/r17_step/): between two full-shard scans the compute stream ran the two kernels
// back to back -- each a few microseconds of work at the headline's candidate counts, each paying
// a launch and a launch-to-launch dependency gap -- and then a four-byte device-to-host copy of
// the tier word, the largest single item of the tail.  Here the scores stay in LDS between the
// two halves while the list fits (PF_LDS entries; longer lists go through cand_s in global memory
// behind a fence and a workgroup barrier), and thread 0 of workgroup 0 stores the tier word
// straight into a pinned, device-mapped host word.
//
// A score is bit for bit what rescore_bf16_kernel writes: the same per-lane fma chain over the
// lane's D / 64 elements, then wave_sum.  The select is topk_select_counted_kernel<KMAX, 256>'s:
// the same strided walk, the same floor pass for long lists, the same wave pops -- so ties break
// the same way too.
#include "scan_common.h"

namespace symb {

constexpr int PF_NTH = 256;    // threads per workgroup (4 waves: the select's form)
constexpr int PF_LDS = 2048;   // scores kept in LDS (8 KiB)

// Top-k of cs[0 .. n) (ids ci[.]) by one PF_NTH-thread workgroup, as topk_select_counted_kernel;
// the result is valid in wave 0's lanes 0 .. KMAX - 1 (rv, ri).  Every thread of the workgroup
// calls it (barriers inside); ls / li / floor_s: the workgroup's LDS scratch.
template <int KMAX, class SP>
__device__ __forceinline__ void pf_select(SP cs, const int* __restrict__ ci, int n, float* ls,
                                          int* li, float* floor_s, float& rv, int& ri) {
  constexpr int NTH = PF_NTH, NW = NTH / 64, P = NW * KMAX / 64;
  static_assert(NW * KMAX % 64 == 0 && P >= 1, "wave lists must tile wave 0's lanes");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float tv[KMAX];
  int ti[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    tv[i] = -INFINITY;
    ti[i] = -1;
  }
  float floor_v = -INFINITY;
  if (n >= 8 * NTH) {   // (block-uniform) long lists: the KMAX-th largest per-thread maximum
    float mx = -INFINITY;
    int c = tid;
    for (; c + 3 * NTH < n; c += 4 * NTH) {
      float s[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = cs[c + u * NTH];
      mx = fmaxf(fmaxf(mx, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
    }
    for (; c < n; c += NTH) mx = fmaxf(mx, cs[c]);
    float mv[1] = {mx};
    int mi[1] = {0};
    wave_pop_topk<KMAX, 1>(mv, mi, lane, rv, ri);
    if (lane < KMAX) ls[wave * KMAX + lane] = rv;
    __syncthreads();
    if (wave == 0) {
      float pv[P];
      int pi[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        pv[j] = -INFINITY;
        pi[j] = 0;
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float v = ls[lane + 64 * j];
        if (v > pv[P - 1]) topk_insert<P>(pv, pi, v, 0);
      }
      wave_pop_topk<KMAX, P>(pv, pi, lane, rv, ri);
      if (lane == KMAX - 1) *floor_s = rv;
    }
    __syncthreads();
    floor_v = *floor_s;
  }
  int c = tid;
  for (; c + 3 * NTH < n; c += 4 * NTH) {
    float s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = cs[c + u * NTH];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (s[u] >= floor_v && s[u] > tv[KMAX - 1]) topk_insert<KMAX>(tv, ti, s[u], ci[c + u * NTH]);
  }
  for (; c < n; c += NTH) {
    const float s = cs[c];
    if (s >= floor_v && s > tv[KMAX - 1]) topk_insert<KMAX>(tv, ti, s, ci[c]);
  }
  wave_pop_topk<KMAX, KMAX>(tv, ti, lane, rv, ri);
  if (lane < KMAX) {
    ls[wave * KMAX + lane] = rv;
    li[wave * KMAX + lane] = ri;
  }
  __syncthreads();
  if (wave != 0) return;
  float pv[P];
  int pi[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    pv[j] = -INFINITY;
    pi[j] = -1;
  }
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const float v = ls[lane + 64 * j];
    if (v > pv[P - 1]) topk_insert<P>(pv, pi, v, li[lane + 64 * j]);
  }
  wave_pop_topk<KMAX, P>(pv, pi, lane, rv, ri);
}

// X: the shard's bf16 rows [n_rows][D]; Q [NQ][D]; cand_i / cand_s [NQ][cap], cand_n [NQ] (a
// count above cap raises *ovf; the first cap entries are used).  out_s / out_i [NQ][k], k <= KMAX.
// tier / host_word (both or neither): *host_word = *tier, stored by thread 0 of workgroup 0 at
// system scope -- host_word is the device address of a pinned, mapped host word.
template <int D, int KMAX>
__global__ __launch_bounds__(PF_NTH) void prune_finish_kernel(
    const __bf16* __restrict__ X, int n_rows, const __bf16* __restrict__ Q,
    const int* __restrict__ cand_i, const int* __restrict__ cand_n, int cap, float* cand_s, int k,
    float* __restrict__ out_s, int* __restrict__ out_i, int* __restrict__ ovf,
    const int* __restrict__ tier, int* host_word) {
  constexpr int PER = D / 64, NW = PF_NTH / 64;
  __shared__ float sc[PF_LDS];
  __shared__ float ls[NW * KMAX];
  __shared__ int li[NW * KMAX];
  __shared__ float floor_s;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tier != nullptr && q == 0 && tid == 0)
    __hip_atomic_store(host_word, *tier, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int cnt = cand_n[q];
  const int n = min(cnt, cap);
  if (tid == 0 && cnt > cap) *ovf = 1;
  const int* ci = cand_i + (size_t)q * cap;
  float* cs = cand_s + (size_t)q * cap;
  const bool in_lds = n <= PF_LDS;   // (block-uniform)

  // ---- 1. the exact scores (rescore_bf16_kernel's arithmetic: one wave per candidate, U row
  //         gathers in flight per wave, PER elements per lane) ----
  float qv[PER];
  {
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(Q + (size_t)q * D + PER * lane);
#pragma unroll
    for (int i = 0; i < PER / 2; ++i) {
      const uint32_t w = qp[i];
      qv[2 * i] = __uint_as_float(w << 16);
      qv[2 * i + 1] = __uint_as_float(w & 0xffff0000u);
    }
  }
  constexpr int U = 8;
  for (int c0 = wave * U; c0 < n; c0 += NW * U) {
    uint32_t w[U][PER / 2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = min(c0 + u, n - 1);
      const int row = min(max(ci[c], 0), n_rows - 1);   // (a valid id is unchanged)
      const uint32_t* xp = reinterpret_cast<const uint32_t*>(X + (size_t)row * D + PER * lane);
#pragma unroll
      for (int i = 0; i < PER / 2; ++i) w[u][i] = xp[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float d = 0.f;
#pragma unroll
      for (int i = 0; i < PER / 2; ++i) {
        d = fmaf(qv[2 * i], __uint_as_float(w[u][i] << 16), d);
        d = fmaf(qv[2 * i + 1], __uint_as_float(w[u][i] & 0xffff0000u), d);
      }
      d = wave_sum(d);
      if (lane == 0 && c0 + u < n) {
        cs[c0 + u] = d;   // (diagnostics read the scores; the long-list select below too)
        if (in_lds) sc[c0 + u] = d;
      }
    }
  }
  if (!in_lds) __threadfence();   // the other waves' scores, read back from global memory
  __syncthreads();

  // ---- 2. the top k ----
  float rv;
  int ri;
  if (in_lds)
    pf_select<KMAX>(static_cast<const float*>(sc), ci, n, ls, li, &floor_s, rv, ri);
  else
    pf_select<KMAX>(static_cast<const float*>(cs), ci, n, ls, li, &floor_s, rv, ri);
  if (wave == 0 && lane < k) {
    out_s[(size_t)q * k + lane] = rv;
    out_i[(size_t)q * k + lane] = ri;
  }
}

}  // namespace symb

using namespace symb;

// The pruned search's finish (prune_finish_kernel): k <= kmax = 16; tier / host_word both or
// neither; *ovf is raised, never cleared here.
int symb_prune_finish(const void* X, int n_rows, const void* Q, int NQ, int dim, const int* cand_i,
                      const int* cand_n, int cap, float* cand_s, int kmax, int k, float* out_s,
                      int* out_i, int* ovf, const int* tier, int* host_word, hipStream_t st) {
  if (NQ <= 0) return 0;
  if (kmax != 16 || k <= 0 || k > kmax || cap <= 0 || n_rows <= 0) return -1;
  if (X == nullptr || Q == nullptr || cand_i == nullptr || cand_n == nullptr ||
      cand_s == nullptr || out_s == nullptr || out_i == nullptr || ovf == nullptr)
    return -1;
  if ((tier == nullptr) != (host_word == nullptr)) return -1;
#define L(D_)                                                                                     \
  hipLaunchKernelGGL((prune_finish_kernel<D_, 16>), dim3(NQ), dim3(PF_NTH), 0, st,                 \
                     (const __bf16*)X, n_rows, (const __bf16*)Q, cand_i, cand_n, cap, cand_s, k,  \
                     out_s, out_i, ovf, tier, host_word)
  if (dim == 384) L(384);
  else if (dim == 768) L(768);
  else if (dim == 1024) L(1024);
  else return -1;
#undef L
  return (int)hipGetLastError();
}
