// Exact cosine top-k under a row mask: the 256-query register top-k scan of index_topk.hip, made
// to walk only the 64-row tiles that hold an allowed row and to ignore disallowed rows in them.
//
// Mask: one bit per row, little-endian within a byte (numpy.packbits(bitorder="little")), the
// byte count padded to a multiple of 8, so a 64-row tile is one aligned 64-bit word; bit r % 64
// of word r / 64 set = row r may be returned.  Rows at or past n_valid are disallowed whatever
// their bits say.
//
//  * filter_tiles_kernel (two launches: count, then scatter) turns the mask into the ascending
//    list of live tiles (word non-zero after clearing the bits at or past n_valid) and their
//    count n_live, both in device memory.  Deterministic: a prefix sum over per-workgroup counts
//    and an ordered in-workgroup scan, no atomic append.
//  * index_scan_filter_kernel is index_scan_topk_kernel's design (8 waves, queries resident as
//    MFMA B fragments, LDS-DMA ring with counted vmcnt and a raw barrier, hand-counted
//    ds_read_b128 fragment pipeline, per-lane register top-k, the same candidate layout) with
//    three differences:
//      - workgroup rb walks the slice [rb * per, min((rb + 1) * per, n_live)) of the live-tile
//        list, per = ceil(n_live / n_rblk), n_live read from device memory (the host sizes the
//        grid from "every tile live" and never reads n_live back);
//      - the DMA source of a ring slot is X + tile * 64 * D with tile read from the list, a
//        wave-uniform base beside the unchanged per-lane offsets;
//      - the tile's mask word is wave-uniform, and every accumulator whose row bit is clear goes
//        to -inf before the max test, so a disallowed row neither enters a list nor raises the
//        threshold.
//    `stride` walks every stride-th entry of the slice only (the seed pass of the shard).
//
// Tile indices and mask words are wave-uniform, so they are read by scalar loads.  Those are
// issued by hand right after the barrier and waited for at the END of the interval (one interval
// ahead of their use): a compiler-placed scalar load would be waited for with lgkmcnt(0) wherever
// its value is first used, in the middle of the counted ds_read pipeline.  A scalar load in flight
// only makes the counted lgkmcnt waits of the fragment pipeline stricter (the counter covers both),
// never looser.
#include "scan_common.h"

#include <algorithm>
#include <type_traits>

namespace symb {

// ---- live-tile list (live_word: scan_common.h) -------------------------------------------------
constexpr int FT_THREADS = 256;

// block-wide sum of one int per thread (FT_THREADS threads), returned to every thread
__device__ __forceinline__ int ft_block_sum(int v, int* lds4) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();   // (lds4 may still be read from an earlier call)
  if (lane == 0) lds4[wave] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

// PASS 0: blk_cnt[b] = live words of workgroup b's contiguous chunk.
// PASS 1: tiles[prefix(b) ...] = the chunk's live word indices in ascending order; the last
// workgroup writes n_live.
template <int PASS>
__global__ __launch_bounds__(FT_THREADS) void filter_tiles_kernel(
    const uint64_t* __restrict__ mask, int n_words, int n_valid, int* __restrict__ blk_cnt,
    int* __restrict__ tiles, int* __restrict__ n_live) {
  __shared__ int lds4[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = (n_words + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min((int)blockIdx.x * chunk, n_words), hi = min(lo + chunk, n_words);
  if constexpr (PASS == 0) {
    int c = 0;
    for (int i = lo + tid; i < hi; i += FT_THREADS) c += live_word(mask[i], i, n_valid) != 0;
    c = ft_block_sum(c, lds4);
    if (tid == 0) blk_cnt[blockIdx.x] = c;
  } else {
    int c = 0;
    for (int b = tid; b < (int)blockIdx.x; b += FT_THREADS) c += blk_cnt[b];
    int base = ft_block_sum(c, lds4);
    for (int i0 = lo; i0 < hi; i0 += FT_THREADS) {
      const int i = i0 + tid;
      const bool live = i < hi && live_word(mask[i], i, n_valid) != 0;
      const uint64_t bal = __ballot(live);
      const int below = __popcll(bal & ((1ull << lane) - 1));
      __syncthreads();
      if (lane == 0) lds4[wave] = __popcll(bal);
      __syncthreads();
      int off = base;
      for (int w = 0; w < wave; ++w) off += lds4[w];
      if (live) tiles[off + below] = i;
      base += lds4[0] + lds4[1] + lds4[2] + lds4[3];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *n_live = base;
  }
}

// (the hand-issued scalar loads of the header note, sload_i32 / sload_u64 / swait: scan_common.h)

// Template parameters as index_scan_topk_kernel (index_topk.hip).  A list entry is a 64-row tile;
// a barrier interval covers TR = 64 rows at D = 384 and 32 rows at D = 768 / 1024, where one list
// entry is two intervals (IPE).
template <int D, bool MFMA_32, int KMAX, int NS, int AUX>
__global__ __launch_bounds__(512) void index_scan_filter_kernel(
    const __bf16* __restrict__ X, int n_valid, const int* __restrict__ tiles,
    const int* __restrict__ n_live_p, const uint64_t* __restrict__ mask, int stride,
    const __bf16* __restrict__ Q, int NQ, int n_qblk, int xcd, const float* __restrict__ thr_init,
    float* __restrict__ cand_s, int* __restrict__ cand_i, const int* __restrict__ gate) {
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
  // row of accumulator register r within the sub-tile = lane_row + acc_reg_row(r)
  const int lane_row = MFMA_32 ? 4 * (lane >> 5) : 4 * (lane >> 4);
  // bits: the sub-tile's SUB mask bits (wave-uniform), bit j = row row0 + j allowed
  auto topk_update = [&](Acc& acc, int row0, uint32_t bits) {
    constexpr uint32_t FULL = MFMA_32 ? 0xffffffffu : 0xffffu;
    if (bits != FULL) {
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

  // Scalar state, one interval ahead: t_cur / w_cur = tile and mask word of interval t, t_nxt =
  // tile of interval t + 1, t_pf = tile of the interval prefetched during t (t + NS - 1, clamped
  // to the slice's last interval: re-loading it keeps the counted vmcnt exact).
  int t_cur = 0, t_nxt = 0, t_pf = 0;
  uint64_t w_cur = 0;
  if (n_iv > 0) {
    int dummy = 0;
    sload_i32(t_cur, tile_ptr(0));
    sload_i32(t_nxt, tile_ptr(1));
    swait(t_cur, t_nxt, w_cur);
    sload_i32(t_pf, tile_ptr(NS - 1));
    sload_u64(w_cur, mask + t_cur);
    swait(t_pf, dummy, w_cur);
    w_cur = live_word(w_cur, t_cur, n_valid);
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
    sload_i32(n_nxt, tile_ptr(t + 2));
    sload_i32(n_pf, tile_ptr(t + NS));
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

    swait(n_nxt, n_pf, n_w);
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

}  // namespace symb

using namespace symb;

// mask: [n_words] 64-bit words; tiles: [>= max(n_words, 1)] ints; blk_cnt: [>= 256] ints of
// workspace; n_live: one int.  Two launches (count, scatter); nothing is read back.
int symb_filter_tiles(const void* mask, int n_words, int n_valid, int* blk_cnt, int* tiles,
                      int* n_live, hipStream_t st) {
  if (n_words < 0) return -1;
  const int grid = std::max(1, std::min(256, (n_words + FT_THREADS - 1) / FT_THREADS));
  hipLaunchKernelGGL(filter_tiles_kernel<0>, dim3(grid), dim3(FT_THREADS), 0, st,
                     (const uint64_t*)mask, n_words, n_valid, blk_cnt, tiles, n_live);
  hipLaunchKernelGGL(filter_tiles_kernel<1>, dim3(grid), dim3(FT_THREADS), 0, st,
                     (const uint64_t*)mask, n_words, n_valid, blk_cnt, tiles, n_live);
  return (int)hipGetLastError();
}

template <int D, bool M32, int KMAX, int NS, int AUX>
static int launch_filter(const void* X, int n_valid, const int* tiles, const int* n_live,
                         const void* mask, int stride, int n_rblk, const void* Q, int NQ,
                         int n_qblk, int xcd, const float* thr, float* cs, int* ci,
                         hipStream_t st, const int* gate) {
  auto kern = index_scan_filter_kernel<D, M32, KMAX, NS, AUX>;
  constexpr int lds = NS * (M32 ? 64 : 32) * D * 2;
  set_max_lds<index_scan_filter_kernel<D, M32, KMAX, NS, AUX>>(lds);
  hipLaunchKernelGGL(kern, dim3(n_rblk * n_qblk), dim3(512), lds, st, (const __bf16*)X, n_valid,
                     tiles, n_live, (const uint64_t*)mask, stride, (const __bf16*)Q, NQ, n_qblk,
                     xcd, thr, cs, ci, gate);
  return (int)hipGetLastError();
}

template <int D, bool M32, int NS>
static int filter_dispatch(int kmax, int aux, const void* X, int n_valid, const int* tiles,
                           const int* n_live, const void* mask, int stride, int n_rblk,
                           const void* Q, int NQ, int n_qblk, int xcd, const float* thr, float* cs,
                           int* ci, hipStream_t st, const int* gate) {
#define SYMB_L(K, A) launch_filter<D, M32, K, NS, A>(X, n_valid, tiles, n_live, mask, stride, n_rblk, Q, NQ, n_qblk, xcd, thr, cs, ci, st, gate)
  if (kmax == 16) return aux ? SYMB_L(16, 2) : SYMB_L(16, 0);
  return aux ? SYMB_L(32, 2) : SYMB_L(32, 0);
#undef SYMB_L
}

// X: [>= round_up(n_valid, 64), D] bf16 unit rows; Q: [NQ, D] bf16 unit rows.
// tiles / n_live: symb_filter_tiles' output for `mask` at this n_valid (every entry a tile
// below ceil(n_valid / 64)); mask: the words filter_tiles read.
// cand_*: [NQ][n_rblk][lists][kmax] (symb_topk_geometry), merged by symb_topk_merge.
// stride >= 1: walk every stride-th entry of each workgroup's slice.
// gate (optional, device int): the scan runs only if *gate != 0.
int symb_index_scan_filter(const void* X, int n_valid, int D, const int* tiles, const int* n_live,
                           const void* mask, int stride, int n_rblk, const void* Q, int NQ,
                           int kmax, float* cand_s, int* cand_i, hipStream_t st,
                           const float* thr_init, int xcd, const int* gate) {
  if (NQ <= 0 || n_rblk <= 0) return 0;
  if (stride < 1 || n_valid < 0 || (kmax != 16 && kmax != 32)) return -1;
  if (!tiles || !n_live || !mask) return -1;
  const int qpb = D == 384 ? 256 : 128;
  const int n_qblk = (NQ + qpb - 1) / qpb;
  const int aux = n_qblk == 1 ? 2 : 0;   // non-temporal when each index row is read by one block
#define SYMB_ARGS kmax, aux, X, n_valid, tiles, n_live, mask, stride, n_rblk, Q, NQ, n_qblk, xcd, thr_init, cand_s, cand_i, st, gate
  if (D == 384) return filter_dispatch<384, true, 3>(SYMB_ARGS);
  if (D == 768) return filter_dispatch<768, false, 3>(SYMB_ARGS);
  if (D == 1024) return filter_dispatch<1024, false, 2>(SYMB_ARGS);
#undef SYMB_ARGS
  return -1;
}
