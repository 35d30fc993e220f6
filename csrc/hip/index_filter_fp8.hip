// The masked e4m3 list scan under ONE row mask: index_scan_filter_fp8_kernel (fp8_filter_scan.h)
// at GROUPED = false, its entry point, and the ring depth the tests bracket.
#include "fp8_filter_scan.h"

using namespace symb;

// LDS ring depth (NS) of the masked scan at width D, -1 for a width it does not serve: the slice
// lengths the tests bracket
int symb_filter_fp8_ring_depth(int D) {
  switch (D) {
    case 256: return Fp8Cfg<256>::NS;
    case 384: return Fp8Cfg<384>::NS;
    case 512: return Fp8Cfg<512>::NS;
    case 768: return Fp8Cfg<768>::NS;
    case 1024: return Fp8Cfg<1024>::NS;
  }
  return -1;
}

// X: [>= round_up(n_valid, 64), D] e4m3 rows (scale S); Q: [NQ, D] e4m3 queries (scale S).
// tiles / n_live: symb_filter_tiles' output for `mask` at this n_valid (every entry a tile
// below ceil(n_valid / 64)); mask: the words filter_tiles read.
// cand_*: [NQ][n_rblk][2][kmax] raw accumulators (S^2 * cosine), merged by symb_topk_merge;
// thr_init in the same units.  stride >= 1: walk every stride-th entry of each slice.
int symb_index_scan_filter_fp8(const void* X, int n_valid, int D, const int* tiles,
                               const int* n_live, const void* mask, int stride, int n_rblk,
                               const void* Q, int NQ, int kmax, float* cand_s, int* cand_i,
                               hipStream_t st, const float* thr_init, int xcd,
                               const int* gate) {
  return index_scan_filter_fp8<false>(X, n_valid, D, tiles, n_live, mask, nullptr, stride, n_rblk,
                                      Q, NQ, kmax, cand_s, cand_i, st, thr_init, xcd, gate);
}
