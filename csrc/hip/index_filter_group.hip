// Exact cosine top-k under a row mask PER QUERY: index_scan_filter_kernel (filter_scan.h) at
// GROUPED = true, and its entry point.  One scan of the rows serves a 256-query block whose
// queries fall into up to MASK_GROUPS = 8 different filters.
#include "filter_scan.h"

using namespace symb;

// As symb_index_scan_filter (index_filter.hip), with the mask a word per group:
// mask8: [n_words][8] 64-bit words, slot g of tile t = group g's mask word;
// qgroup: [NQ] ints, query q's group (only its low three bits are used);
// tiles / n_live: symb_filter_tiles' output for the OR of the eight slots at this n_valid.
int symb_index_scan_filter_group(const void* X, int n_valid, int D, const int* tiles,
                                 const int* n_live, const void* mask8, const int* qgroup,
                                 int stride, int n_rblk, const void* Q, int NQ, int kmax,
                                 float* cand_s, int* cand_i, hipStream_t st, const float* thr_init,
                                 int xcd, const int* gate) {
  return index_scan_filter<true>(X, n_valid, D, tiles, n_live, mask8, qgroup, stride, n_rblk, Q,
                                 NQ, kmax, cand_s, cand_i, st, thr_init, xcd, gate);
}
