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
//  * index_scan_filter_kernel (filter_scan.h) walks that list; this file instantiates its
//    single-mask form (GROUPED = false) and holds its entry point.
#include "filter_scan.h"

#include <algorithm>

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
  return index_scan_filter<false>(X, n_valid, D, tiles, n_live, mask, nullptr, stride, n_rblk, Q,
                                  NQ, kmax, cand_s, cand_i, st, thr_init, xcd, gate);
}
