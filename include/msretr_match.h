/* libmsretr -- match modes: "all of these words", "at least m of them" (same library, same
 * conventions as msretr.h, whose msr_engine this call takes).  A header of its own: the call was added without changing any
 * existing one and without a new MSR_ABI_VERSION -- a library that lacks it fails to load by symbol.
 *
 * msr_match_sets: document sets that COUNT, the producer beside msr_term_sets of the rows that the *_within calls,
 * msr_dense_topk_grouped and msr_facet_counts consume.  A row has groups, a group has terms: row r's groups are
 * [row_group_off[r], row_group_off[r + 1]) (numbered across the call), group g's terms group_terms[group_term_off[g] ..
 * group_term_off[g + 1]) (int32 offsets from 0; n_rows + 1 and n_groups + 1 of them, n_groups = row_group_off[n_rows]).  A
 * document FILLS a group when it stands in the bound posting list D(t) of at least one of the group's terms.  Row r of
 * out_bits (rows out_stride words apart, the layout of msretr.h: document d is bit d & 31 of word d >> 5) becomes
 *     base(r)  AND  { d : the number of row r's groups that d fills  >=  row_need[r] }
 * with D(t) and base(r) exactly msr_term_sets'.  Conventions:
 *   - a term outside [0, n_terms), or with an empty list, contributes nothing; its group still counts among the row's groups
 *     (a word the index lacks is a group that no document fills); a group may hold any number of terms, none included;
 *   - a document in several terms of one group fills it once; the same term in two groups fills both;
 *   - row_need[r] <= 0 gives base(r); row_need[r] above the row's number of groups gives the empty row (so does any
 *     row_need[r] > 0 on a row without groups);
 *   - a row of more than MSR_MATCH_MAX_GROUPS groups is the empty row (a host should refuse it earlier: it is
 *     MSR_MAX_QUERY_TERMS, what a query can score);
 *   - base(r) follows msr_term_sets' rules: row_base[r] == -1, or n_base == 0 (base_bits / row_base are then not read), is
 *     every document; a value in [0, n_base) picks that row of base_bits; any other value is the empty set, and no row
 *     outside the n_base rows is read.
 * Every word [0, ceil(n_docs / 32)) of every row is written (the buffer need not be zeroed), bits at or above n_docs are 0,
 * words [ceil(n_docs / 32), out_stride) are not touched.  out_bits must not alias base_bits.  Repeated calls give the same
 * bytes.  The call only enqueues on `stream` (every array is a device pointer; offsets and needs are read on the device): one
 * kernel per 32768 rows, no global atomic, no memset, and no scratch in the engine.  Refused with MSR_ERR_INVALID before any
 * launch, outputs untouched: n_rows < 0; with n_rows > 0 a NULL out_bits, row_group_off, group_term_off or row_need;
 * out_stride < ceil(n_docs / 32); n_base < 0; with n_base > 0 a NULL base_bits or row_base, or base_stride <
 * ceil(n_docs / 32).  (group_terms may be NULL when no group holds a term.)  MSR_ERR_NOT_BOUND without postings.  n_rows == 0
 * succeeds and launches nothing.  Cost: 4 bytes read per posting of every listed term (less what a span of
 * MSR_TERMSET_SPAN_DOCS documents skips once none of its base documents can still reach the row's need) plus the base rows,
 * 4 ceil(n_docs / 32) bytes written per row. */
#ifndef MSRETR_MATCH_H
#define MSRETR_MATCH_H

#include "msretr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSR_MATCH_MAX_GROUPS 64 /* msr_match_sets: groups of one row (== MSR_MAX_QUERY_TERMS) */

int msr_match_sets(msr_engine* e, int32_t n_rows, const int32_t* row_group_off, const int32_t* group_term_off,
                   const int32_t* group_terms, const int32_t* row_need,
                   const uint32_t* base_bits, int32_t n_base, int64_t base_stride, const int32_t* row_base,
                   uint32_t* out_bits, int64_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MSRETR_MATCH_H */
