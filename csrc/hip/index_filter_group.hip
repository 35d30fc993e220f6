// Exact cosine top-k under a row mask PER QUERY: index_scan_filter_kernel (index_filter.hip) with
// the tile's mask word a per-lane value instead of a wave-uniform one, so one scan of the rows
// serves a 256-query block whose queries fall into up to MASK_GROUPS = 8 different filters.
//
// Inputs beside index_scan_filter_kernel's:
//   * mask8: uint64 [n_words][8], 64 bytes per 64-row tile; slot g of a tile is the mask word of
//     group g (bit r % 64 = row r allowed for the queries of group g), unused slots 0.
//   * qgroup: int32 [NQ], the group of each query.  A lane reads qgroup[min(query, NQ - 1)] & 7
//     once, beside thr_init; the & 7 keeps any value inside the tile's 64 bytes.
//   * tiles / n_live: filter_tiles of the OR of the groups' words.  A tile that is live for one
//     group and empty for another sends the other group's lanes to -inf, nothing more.
//
// In both MFMA shapes every accumulator of a lane belongs to one query (qlocal = lane & 31 or
// lane & 15), so "the query's mask" is a per-lane value and topk_update's masking arithmetic --
// already vector arithmetic there, the lane's row offset being per-lane -- carries over.  The
// MFMA chain, the LDS-DMA ring, the fragment pipeline and the register top-k are
// index_scan_filter_kernel's, and an MFMA column does not depend on its neighbours, so a row
// scores here bit for bit what it scores there.
//
// Per barrier interval the eight words of the NEXT tile come by one hand-issued s_load_dwordx16
// of mask8 + 8 * t_nxt, issued where index_scan_filter_kernel issues its s_load_dwordx2 and waited
// for at the end of the interval with the tile indices.  The lane's word is then picked into a
// VGPR pair by a compare-and-select chain over its group id (14 v_cndmask_b32), cut at n_valid the
// way live_word cuts it (the cut is wave-uniform: the tile is), and only that pair crosses the
// barrier -- 16 SGPRs are in flight during an interval, not 32.
//
// The all-rows-allowed shortcut of topk_update is a WAVE VOTE (skip the masking selects only if
// every lane's bits are full), not a per-lane branch: the masking is sixteen (or four) selects,
// which a per-lane `if` would be if-converted into anyway -- paying them on every sub-tile -- or
// would wrap in an exec-mask save / restore inside the counted ds_read pipeline.  The vote is one
// v_cmp and a scalar branch, keeps the dense case (must_not filters: almost every word full for
// every group) on the unmasked path, and cannot change a score: a lane whose bits are full takes
// no select under either form.
//
// Register budget: three VGPRs more than index_scan_filter_kernel (the word pair and the group
// id).  PF (fragment reads in flight) is that kernel's at every instantiation; none uses scratch
// (profiles/r14_group_filter/resource_usage.md).
// (MASK_GROUPS, sload_mask8, swait_mask8, pick_word: mask_group.h, shared with the fp8 form)
#include "mask_group.h"

#include <algorithm>
#include <type_traits>

namespace symb {

// Template parameters and tile / interval geometry as index_scan_filter_kernel.
template <int D, bool MFMA_32, int KMAX, int NS, int AUX>
__global__ __launch_bounds__(512) void index_scan_filter_group_kernel(
    const __bf16* __restrict__ X, int n_valid, const int* __restrict__ tiles,
    const int* __restrict__ n_live_p, const uint64_t* __restrict__ mask8,
    const int* __restrict__ qgroup, int stride, const __bf16* __restrict__ Q, int NQ, int n_qblk,
    int xcd, const float* __restrict__ thr_init, float* __restrict__ cand_s,
    int* __restrict__ cand_i, const int* __restrict__ gate) {
  // gate (optional): run only if *gate != 0 (as index_scan_filter_kernel)
  if (gate != nullptr && *gate == 0) return;
  constexpr int CPR = D / 8;                          // 16-byte chunks per row
  constexpr int SUB = MFMA_32 ? 32 : 16;              // rows per MFMA chain (sub-tile)
  constexpr int TR = 2 * SUB;                         // rows per barrier interval
  constexpr int IPE = 64 / TR;                        // intervals per list entry
  constexpr int TILE_BYTES = TR * D * 2;
  constexpr int SUB_BYTES = SUB * D * 2;
  constexpr int LOADS = TILE_BYTES / (1024 * TOPK_WAVES);  // glds per wave per interval
  constexpr int DMA_EVERY = 4;                             // MFMA steps between DMA pieces
  static_assert(TILE_BYTES % (1024 * TOPK_WAVES) == 0, "tile must split evenly over waves");
  static_assert(NS >= 2 && NS * TILE_BYTES <= 160 * 1024, "LDS ring exceeds the CU's 160 KiB");
  constexpr int QW = MFMA_32 ? 32 : 16;               // queries per wave
  constexpr int NKS = MFMA_32 ? D / 16 : D / 32;      // MFMA k-steps over D
  constexpr int LISTS = MFMA_32 ? 2 : 4;
  constexpr int M = MFMA_32 ? 8 : 4;                  // period of the per-lane fragment offsets
  // fragment reads in flight: index_scan_filter_kernel's
  constexpr int PF = (KMAX <= 16 || D == 768) ? 6 : (D == 1024 ? 2 : 3);
  using Acc = typename std::conditional<MFMA_32, f32x16, f32x4>::type;
  constexpr int NR = MFMA_32 ? 16 : 4;                // accumulator registers per lane
  static_assert(LOADS * DMA_EVERY <= NKS, "DMA pieces must fit the first chain");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lb = xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int qb = lb % n_qblk, rb = lb / n_qblk;
  const int n_rblk = gridDim.x / n_qblk;

  // ---- this workgroup's slice of the live-tile list ----
  const int n_live = __builtin_amdgcn_readfirstlane(*n_live_p);
  const int per = (n_live + n_rblk - 1) / n_rblk;
  const int slice_begin = __builtin_amdgcn_readfirstlane(min(rb * per, n_live));
  const int slice_len = min(per, n_live - slice_begin);
  const int n_ent = slice_len > 0 ? (slice_len + stride - 1) / stride : 0;   // entries walked
  const int n_iv = __builtin_amdgcn_readfirstlane(n_ent * IPE);              // barrier intervals
  // interval iv (clamped to the last one) -> its entry's position in the list / its first row
  // within that entry's tile
  auto tile_ptr = [&](int iv) {
    return tiles + slice_begin + (min(iv, n_iv - 1) / IPE) * stride;
  };
  auto half_row = [&](int iv) { return (min(iv, n_iv - 1) % IPE) * TR; };

  // ---- query fragments (B operand) ----
  const int qlocal = MFMA_32 ? (lane & 31) : (lane & 15);
  const int query = qb * (QW * TOPK_WAVES) + wave * QW + qlocal;
  const __bf16* qp = Q + (size_t)min(query, NQ - 1) * D;
  bf16x8 qf[NKS];
  load_query_frags<D, MFMA_32>(qf, qp, lane);

  // ---- per-thread DMA source offsets within an interval (identical for every interval) ----
  uint32_t goff[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    const int s = (i * TOPK_WAVES + wave) * 64 + lane;  // LDS 16-byte slot filled
    const int row = s / CPR, pc = s % CPR;
    const int c = pc ^ (row & 15);
    goff[i] = (uint32_t)(row * D + c * 8);
  }
  // row_base: first row of the interval (wave-uniform); slot: interval number (ring position)
  auto issue_piece = [&](int row_base, int slot, int i) {
    const __bf16* base = X + (size_t)row_base * D;
    char* dst = smem + (slot % NS) * TILE_BYTES;
    glds16_aux<AUX>(base + goff[i], dst + ((i * TOPK_WAVES + wave) * 64) * 16);
  };

  // ---- per-lane LDS fragment offsets within a sub-tile (see FragChain) ----
  const uint32_t lds_smem = lds_addr(smem);
  uint32_t voff[M];
  if constexpr (MFMA_32) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int m = 0; m < M; ++m) voff[m] = (uint32_t)(r * D * 2 + (((2 * m + h) ^ (r & 15)) << 4));
  } else {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int m = 0; m < M; ++m) voff[m] = (uint32_t)(r * D * 2 + (((4 * m + g) ^ r) << 4));
  }

  float tv[KMAX];
  int ti[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    tv[i] = -INFINITY;
    ti[i] = -1;
  }
  // thr_init[q] (optional): a lower bound on query q's final k-th ALLOWED score
  float thr = thr_init ? thr_init[min(query, NQ - 1)] : -INFINITY;
  // the lane's mask group (padded lanes take the last query's, like its fragments)
  const int grp = qgroup[min(query, NQ - 1)] & (MASK_GROUPS - 1);
  // row of accumulator register r within the sub-tile = lane_row + acc_reg_row(r)
  const int lane_row = MFMA_32 ? 4 * (lane >> 5) : 4 * (lane >> 4);
  // bits: the sub-tile's SUB mask bits of THIS LANE's group, bit j = row row0 + j allowed
  auto topk_update = [&](Acc& acc, int row0, uint32_t bits) {
    constexpr uint32_t FULL = MFMA_32 ? 0xffffffffu : 0xffffu;
    if (__any(bits != FULL)) {   // wave vote (header note)
      const uint32_t lbits = bits >> lane_row;
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (!((lbits >> acc_reg_row<MFMA_32>(r)) & 1u)) acc[r] = -INFINITY;
    }
    float mx = acc[0];
#pragma unroll
    for (int r = 1; r < NR; ++r) mx = fmaxf(mx, acc[r]);
    if (mx > thr) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (acc[r] > thr) {
          // (KMAX = 32: the in-place form; the parallel one's second copy of the list spills)
          if constexpr (KMAX > 16)
            topk_insert<KMAX>(tv, ti, acc[r], row0 + lane_row + acc_reg_row<MFMA_32>(r));
          else
            topk_insert_par<KMAX>(tv, ti, acc[r], row0 + lane_row + acc_reg_row<MFMA_32>(r));
          thr = fmaxf(thr, tv[KMAX - 1]);
        }
      }
    }
  };

  // Scalar state, one interval ahead, as index_scan_filter_kernel; w_cur is the LANE's mask word
  // of interval t's tile (a VGPR pair).
  int t_cur = 0, t_nxt = 0, t_pf = 0;
  uint64_t w_cur = 0;
  if (n_iv > 0) {
    int dummy = 0;
    uint64_t none = 0;
    u32x16 w8;
    sload_i32(t_cur, tile_ptr(0));
    sload_i32(t_nxt, tile_ptr(1));
    swait(t_cur, t_nxt, none);
    sload_i32(t_pf, tile_ptr(NS - 1));
    sload_mask8(w8, mask8 + (size_t)MASK_GROUPS * t_cur);
    swait_mask8(t_pf, dummy, w8);
    w_cur = live_word(pick_word(w8, grp), t_cur, n_valid);
#pragma unroll
    for (int p = 0; p < NS - 1; ++p) {
      static_assert(NS <= 3, "the prologue knows the tiles of intervals 0 and 1 only");
      const int row_base = (p == 0 ? t_cur : t_nxt) * 64 + half_row(p);
#pragma unroll
      for (int i = 0; i < LOADS; ++i) issue_piece(row_base, p, i);
    }
  }
  constexpr int R = PF + 1;
  bf16x8 a[R];
  for (int t = 0; t < n_iv; ++t) {
    // interval t landed for this wave once only the (NS-2) younger intervals' loads remain
    wait_vmcnt<LOADS * (NS - 2)>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // next interval's scalar state (waited for at the end of this interval)
    int n_nxt, n_pf;
    u32x16 n_w8;
    sload_i32(n_nxt, tile_ptr(t + 2));
    sload_i32(n_pf, tile_ptr(t + NS));
    sload_mask8(n_w8, mask8 + (size_t)MASK_GROUPS * t_nxt);

    const uint32_t base0 = lds_smem + (uint32_t)((t % NS) * TILE_BYTES);
    const uint32_t base1 = base0 + SUB_BYTES;
    const int h0 = half_row(t);
    const int row0 = t_cur * 64 + h0;
    const uint32_t wbits = (uint32_t)(w_cur >> h0);   // this interval's TR mask bits (low end)
    const uint32_t bits0 = MFMA_32 ? wbits : (wbits & 0xffffu);
    const uint32_t bits1 = MFMA_32 ? (uint32_t)(w_cur >> 32) : ((wbits >> 16) & 0xffffu);

    Acc acc0, acc1;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      acc0[r] = 0.f;
      acc1[r] = 0.f;
    }
    frag_prologue<0, PF, M, R>(a, voff, base0);
    const int pf_row = t_pf * 64 + half_row(t + NS - 1);
    const int tnext = t + NS - 1;
    auto dma = [&](int i) { issue_piece(pf_row, tnext, i); };
    FragChain<0, NKS, PF, M, MFMA_32, DMA_EVERY, LOADS>::run(acc0, a, qf, voff, base0, dma);
    frag_prologue<0, PF, M, R>(a, voff, base1);   // sub-tile 1 reads fly during top-k of sub 0
    topk_update(acc0, row0, bits0);
    FragChain<0, NKS, PF, M, MFMA_32>::run(acc1, a, qf, voff, base1);
    topk_update(acc1, row0 + SUB, bits1);

    swait_mask8(n_nxt, n_pf, n_w8);
    t_cur = t_nxt;
    t_nxt = n_nxt;
    t_pf = n_pf;
    w_cur = live_word(pick_word(n_w8, grp), t_cur, n_valid);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the tail prefetches before exit

  if (query < NQ) {
    const int list = MFMA_32 ? (lane >> 5) : (lane >> 4);
    const size_t base = (((size_t)query * n_rblk + rb) * LISTS + list) * KMAX;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      cand_s[base + i] = tv[i];
      cand_i[base + i] = ti[i];
    }
  }
}

}  // namespace symb

using namespace symb;

template <int D, bool M32, int KMAX, int NS, int AUX>
static int launch_filter_group(const void* X, int n_valid, const int* tiles, const int* n_live,
                               const void* mask8, const int* qgroup, int stride, int n_rblk,
                               const void* Q, int NQ, int n_qblk, int xcd, const float* thr,
                               float* cs, int* ci, hipStream_t st, const int* gate) {
  auto kern = index_scan_filter_group_kernel<D, M32, KMAX, NS, AUX>;
  constexpr int lds = NS * (M32 ? 64 : 32) * D * 2;
  set_max_lds<index_scan_filter_group_kernel<D, M32, KMAX, NS, AUX>>(lds);
  hipLaunchKernelGGL(kern, dim3(n_rblk * n_qblk), dim3(512), lds, st, (const __bf16*)X, n_valid,
                     tiles, n_live, (const uint64_t*)mask8, qgroup, stride, (const __bf16*)Q, NQ,
                     n_qblk, xcd, thr, cs, ci, gate);
  return (int)hipGetLastError();
}

template <int D, bool M32, int NS>
static int filter_group_dispatch(int kmax, int aux, const void* X, int n_valid, const int* tiles,
                                 const int* n_live, const void* mask8, const int* qgroup,
                                 int stride, int n_rblk, const void* Q, int NQ, int n_qblk,
                                 int xcd, const float* thr, float* cs, int* ci, hipStream_t st,
                                 const int* gate) {
#define SYMB_L(K, A) launch_filter_group<D, M32, K, NS, A>(X, n_valid, tiles, n_live, mask8, qgroup, stride, n_rblk, Q, NQ, n_qblk, xcd, thr, cs, ci, st, gate)
  if (kmax == 16) return aux ? SYMB_L(16, 2) : SYMB_L(16, 0);
  return aux ? SYMB_L(32, 2) : SYMB_L(32, 0);
#undef SYMB_L
}

// As symb_index_scan_filter (index_filter.hip), with the mask a word per group:
// mask8: [n_words][8] 64-bit words, slot g of tile t = group g's mask word;
// qgroup: [NQ] ints, query q's group (only its low three bits are used);
// tiles / n_live: symb_filter_tiles' output for the OR of the eight slots at this n_valid.
int symb_index_scan_filter_group(const void* X, int n_valid, int D, const int* tiles,
                                 const int* n_live, const void* mask8, const int* qgroup,
                                 int stride, int n_rblk, const void* Q, int NQ, int kmax,
                                 float* cand_s, int* cand_i, hipStream_t st, const float* thr_init,
                                 int xcd, const int* gate) {
  if (NQ <= 0 || n_rblk <= 0) return 0;
  if (stride < 1 || n_valid < 0 || (kmax != 16 && kmax != 32)) return -1;
  if (!tiles || !n_live || !mask8 || !qgroup) return -1;
  const int qpb = D == 384 ? 256 : 128;
  const int n_qblk = (NQ + qpb - 1) / qpb;
  const int aux = n_qblk == 1 ? 2 : 0;   // non-temporal when each index row is read by one block
#define SYMB_ARGS kmax, aux, X, n_valid, tiles, n_live, mask8, qgroup, stride, n_rblk, Q, NQ, n_qblk, xcd, thr_init, cand_s, cand_i, st, gate
  if (D == 384) return filter_group_dispatch<384, true, 3>(SYMB_ARGS);
  if (D == 768) return filter_group_dispatch<768, false, 3>(SYMB_ARGS);
  if (D == 1024) return filter_group_dispatch<1024, false, 2>(SYMB_ARGS);
#undef SYMB_ARGS
  return -1;
}
