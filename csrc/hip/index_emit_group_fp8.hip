// The emitting e4m3 scan under a row mask PER QUERY: index_scan_emit_fp8_kernel (fp8_emit.h) at
// GROUPED = true, and its entry point.  It serves fp8 shards at 32 < k <= 128 when the queries of
// one 256-query block fall into up to MASK_GROUPS = 8 filters.
#include "fp8_emit.h"

using namespace symb;

// As symb_index_scan_emit_fp8 (index_emit_fp8.hip), with the mask a word per group as in
// symb_index_scan_filter_group_fp8: mask8 [n_words][8] 64-bit words, qgroup [NQ] ints (low three
// bits), tiles / n_live symb_filter_tiles' output for the OR of the eight slots at this n_valid.
int symb_index_scan_emit_group_fp8(const void* X, int n_valid, int D, const int* tiles,
                                   const int* n_live, const void* mask8, const int* qgroup,
                                   int n_rblk, const void* Q, int NQ, const float* thr,
                                   float* cand_s, int* cand_i, int* cand_n, int cap,
                                   hipStream_t st, int xcd, const int* gate, int zero_cnt) {
  return index_scan_emit_fp8<true>(X, n_valid, D, tiles, n_live, mask8, qgroup, n_rblk, Q, NQ,
                                   thr, cand_s, cand_i, cand_n, cap, st, xcd, gate, zero_cnt);
}
