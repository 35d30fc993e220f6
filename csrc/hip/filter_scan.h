// Exact cosine top-k under a row mask over a bf16 shard, one kernel for both mask forms: the
// 256-query register top-k scan of index_topk.hip, made to walk only the 64-row tiles that hold an
// allowed row and to ignore disallowed rows in them.  index_filter.hip instantiates GROUPED =
// false (one mask for every query) and holds the mask format's note and the live-tile list
// (filter_tiles_kernel); index_filter_group.hip instantiates GROUPED = true (a mask per query).
//
// index_scan_filter_kernel is index_scan_topk_kernel's design (8 waves, queries resident as MFMA B
// fragments, LDS-DMA ring with counted vmcnt and a raw barrier, hand-counted ds_read_b128 fragment
// pipeline, per-lane register top-k, the same candidate layout) with three differences:
//   - workgroup rb walks the slice [rb * per, min((rb + 1) * per, n_live)) of the live-tile list,
//     per = ceil(n_live / n_rblk), n_live read from device memory (the host sizes the grid from
//     "every tile live" and never reads n_live back);
//   - the DMA source of a ring slot is X + tile * 64 * D with tile read from the list, a
//     wave-uniform base beside the unchanged per-lane offsets;
//   - every accumulator whose row bit in the tile's mask word is clear goes to -inf before the
//     max test, so a disallowed row neither enters a list nor raises the threshold.
// `stride` walks every stride-th entry of the slice only (the seed pass of the shard).  The MFMA
// chain is the unfiltered scan's and an MFMA column does not depend on its neighbours, so a row
// scores bit for bit what it scores there, under either mask form.
//
// Tile indices and mask words are wave-uniform, so they are read by scalar loads.  Those are
// issued by hand right after the barrier and waited for at the END of the interval (one interval
// ahead of their use): a compiler-placed scalar load would be waited for with lgkmcnt(0) wherever
// its value is first used, in the middle of the counted ds_read pipeline.  A scalar load in flight
// only makes the counted lgkmcnt waits of the fragment pipeline stricter (the counter covers both),
// never looser.
//
// What GROUPED changes is where the mask word comes from and how the shortcut is taken; every
// such site is an `if constexpr` below.
//  - single mask: `mask` is uint64 [n_words], qgroup is null.  The tile's word comes by one
//    s_load_dwordx2 and stays in SGPRs.
//  - grouped (mask_group.h): `mask` is uint64 [n_words][8], 64 bytes per 64-row tile; slot g of a
//    tile is the mask word of group g (bit r % 64 = row r allowed for the queries of group g),
//    unused slots 0.  qgroup is int32 [NQ]; a lane reads qgroup[min(query, NQ - 1)] & 7 once,
//    beside thr_init; the & 7 keeps any value inside the tile's 64 bytes.  tiles / n_live =
//    filter_tiles of the OR of the groups' words: a tile that is live for one group and empty for
//    another sends the other group's lanes to -inf, nothing more.  In both MFMA shapes every
//    accumulator of a lane belongs to one query (qlocal = lane & 31 or lane & 15), so "the
//    query's mask" is a per-lane value and topk_update's masking arithmetic -- already vector
//    arithmetic, the lane's row offset being per-lane -- carries over.
//    Per barrier interval the eight words of the NEXT tile come by one hand-issued
//    s_load_dwordx16 of mask + 8 * t_nxt, issued where the single-mask form issues its
//    s_load_dwordx2 and waited for at the end of the interval with the tile indices.  The lane's
//    word is then picked into a VGPR pair by a compare-and-select chain over its group id (14
//    v_cndmask_b32), cut at n_valid the way live_word cuts it (the cut is wave-uniform: the tile
//    is), and only that pair crosses the barrier -- 16 SGPRs are in flight during an interval,
//    not 32.
//  - grouped, the all-rows-allowed shortcut of topk_update is a WAVE VOTE (skip the masking
//    selects only if every lane's bits are full), not a per-lane branch: the masking is sixteen
//    (or four) selects, which a per-lane `if` would be if-converted into anyway -- paying them on
//    every sub-tile -- or would wrap in an exec-mask save / restore inside the counted ds_read
//    pipeline.  The vote is one v_cmp and a scalar branch, keeps the dense case (must_not
//    filters: almost every word full for every group) on the unmasked path, and cannot change a
//    score: a lane whose bits are full takes no select under either form.
//
// Register budget: the grouped form takes three VGPRs more (the word pair and the group id).  PF
// (fragment reads in flight) is the same in both forms; no instantiation uses scratch
// (profiles/fold_masked_scans/README.md).
#pragma once
#include "mask_group.h"

#include <type_traits>

namespace symb {

// Template parameters as index_scan_topk_kernel (index_topk.hip).  A list entry is a 64-row tile;
// a barrier interval covers TR = 64 rows at D = 384 and 32 rows at D = 768 / 1024, where one list
// entry is two intervals (IPE).
template <int D, bool MFMA_32, int KMAX, int NS, int AUX, bool GROUPED>
__global__ __launch_bounds__(512) void index_scan_filter_kernel(
    const __bf16* __restrict__ X, int n_valid, const int* __restrict__ tiles,
    const int* __restrict__ n_live_p, const uint64_t* __restrict__ mask,
    const int* __restrict__ qgroup, int stride, const __bf16* __restrict__ Q, int NQ, int n_qblk,
    int xcd, const float* __restrict__ thr_init, float* __restrict__ cand_s,
    int* __restrict__ cand_i, const int* __restrict__ gate) {
  // gate (optional): run only if *gate != 0 -- the exact fallback of a search over a shard with
  // tombstones (index_delete.hip) is enqueued unconditionally and skips itself unless the
  // unmasked route returned a dead row, so no host sync decides it (as index_topk.hip)
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
  // fragment reads in flight: 6 as in the unfiltered scan; at 384 and 1024 the kmax = 32 lists
  // leave fewer registers for the fragment ring (no scratch at any instantiation)
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
  // grouped: the lane's mask group (padded lanes take the last query's, like its fragments)
  int grp = 0;
  if constexpr (GROUPED) grp = qgroup[min(query, NQ - 1)] & (MASK_GROUPS - 1);
  // row of accumulator register r within the sub-tile = lane_row + acc_reg_row(r)
  const int lane_row = MFMA_32 ? 4 * (lane >> 5) : 4 * (lane >> 4);
  // bits: the sub-tile's SUB mask bits (single mask: wave-uniform; grouped: of THIS LANE's
  // group, and the shortcut a wave vote, header note), bit j = row row0 + j allowed
  auto topk_update = [&](Acc& acc, int row0, uint32_t bits) {
    constexpr uint32_t FULL = MFMA_32 ? 0xffffffffu : 0xffffu;
    bool masked;
    if constexpr (GROUPED) masked = __any(bits != FULL);
    else masked = bits != FULL;
    if (masked) {
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

  // Scalar state, one interval ahead: t_cur / w_cur = tile and mask word of interval t (grouped:
  // the LANE's word, a VGPR pair), t_nxt = tile of interval t + 1, t_pf = tile of the interval
  // prefetched during t (t + NS - 1, clamped to the slice's last interval: re-loading it keeps
  // the counted vmcnt exact).
  int t_cur = 0, t_nxt = 0, t_pf = 0;
  uint64_t w_cur = 0;
  if (n_iv > 0) {
    int dummy = 0;
    sload_i32(t_cur, tile_ptr(0));
    sload_i32(t_nxt, tile_ptr(1));
    if constexpr (GROUPED) {
      uint64_t none = 0;
      u32x16 w8;
      swait(t_cur, t_nxt, none);
      sload_i32(t_pf, tile_ptr(NS - 1));
      sload_mask8(w8, mask + (size_t)MASK_GROUPS * t_cur);
      swait_mask8(t_pf, dummy, w8);
      w_cur = live_word(pick_word(w8, grp), t_cur, n_valid);
    } else {
      swait(t_cur, t_nxt, w_cur);
      sload_i32(t_pf, tile_ptr(NS - 1));
      sload_u64(w_cur, mask + t_cur);
      swait(t_pf, dummy, w_cur);
      w_cur = live_word(w_cur, t_cur, n_valid);
    }
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
    uint64_t n_w;
    u32x16 n_w8;
    sload_i32(n_nxt, tile_ptr(t + 2));
    sload_i32(n_pf, tile_ptr(t + NS));
    if constexpr (GROUPED)
      sload_mask8(n_w8, mask + (size_t)MASK_GROUPS * t_nxt);
    else
      sload_u64(n_w, mask + t_nxt);

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

    if constexpr (GROUPED) {
      swait_mask8(n_nxt, n_pf, n_w8);
      n_w = pick_word(n_w8, grp);
    } else {
      swait(n_nxt, n_pf, n_w);
    }
    t_cur = t_nxt;
    t_nxt = n_nxt;
    t_pf = n_pf;
    w_cur = live_word(n_w, t_cur, n_valid);
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

template <bool GROUPED, int D, bool M32, int KMAX, int NS, int AUX>
static int launch_filter(const void* X, int n_valid, const int* tiles, const int* n_live,
                         const void* mask, const int* qgroup, int stride, int n_rblk,
                         const void* Q, int NQ, int n_qblk, int xcd, const float* thr, float* cs,
                         int* ci, hipStream_t st, const int* gate) {
  auto kern = index_scan_filter_kernel<D, M32, KMAX, NS, AUX, GROUPED>;
  constexpr int lds = NS * (M32 ? 64 : 32) * D * 2;
  set_max_lds<index_scan_filter_kernel<D, M32, KMAX, NS, AUX, GROUPED>>(lds);
  hipLaunchKernelGGL(kern, dim3(n_rblk * n_qblk), dim3(512), lds, st, (const __bf16*)X, n_valid,
                     tiles, n_live, (const uint64_t*)mask, qgroup, stride, (const __bf16*)Q, NQ,
                     n_qblk, xcd, thr, cs, ci, gate);
  return (int)hipGetLastError();
}

template <bool GROUPED, int D, bool M32, int NS>
static int filter_dispatch(int kmax, int aux, const void* X, int n_valid, const int* tiles,
                           const int* n_live, const void* mask, const int* qgroup, int stride,
                           int n_rblk, const void* Q, int NQ, int n_qblk, int xcd,
                           const float* thr, float* cs, int* ci, hipStream_t st,
                           const int* gate) {
#define SYMB_L(K, A) launch_filter<GROUPED, D, M32, K, NS, A>(X, n_valid, tiles, n_live, mask, qgroup, stride, n_rblk, Q, NQ, n_qblk, xcd, thr, cs, ci, st, gate)
  if (kmax == 16) return aux ? SYMB_L(16, 2) : SYMB_L(16, 0);
  return aux ? SYMB_L(32, 2) : SYMB_L(32, 0);
#undef SYMB_L
}

// The body of both entry points: argument checks, then the width switch.  qgroup is required
// when GROUPED and ignored (pass null) otherwise.
template <bool GROUPED>
static int index_scan_filter(const void* X, int n_valid, int D, const int* tiles,
                             const int* n_live, const void* mask, const int* qgroup, int stride,
                             int n_rblk, const void* Q, int NQ, int kmax, float* cand_s,
                             int* cand_i, hipStream_t st, const float* thr_init, int xcd,
                             const int* gate) {
  if (NQ <= 0 || n_rblk <= 0) return 0;
  if (stride < 1 || n_valid < 0 || (kmax != 16 && kmax != 32)) return -1;
  if (!tiles || !n_live || !mask || (GROUPED && !qgroup)) return -1;
  const int qpb = D == 384 ? 256 : 128;
  const int n_qblk = (NQ + qpb - 1) / qpb;
  const int aux = n_qblk == 1 ? 2 : 0;   // non-temporal when each index row is read by one block
#define SYMB_ARGS kmax, aux, X, n_valid, tiles, n_live, mask, qgroup, stride, n_rblk, Q, NQ, n_qblk, xcd, thr_init, cand_s, cand_i, st, gate
  if (D == 384) return filter_dispatch<GROUPED, 384, true, 3>(SYMB_ARGS);
  if (D == 768) return filter_dispatch<GROUPED, 768, false, 3>(SYMB_ARGS);
  if (D == 1024) return filter_dispatch<GROUPED, 1024, false, 2>(SYMB_ARGS);
#undef SYMB_ARGS
  return -1;
}

}  // namespace symb
