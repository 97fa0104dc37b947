// msr_facet_table (include/msretr.h): the per-span value dictionaries that msr_bind_facet takes, built
// on the host from one int32 value per document.  Host-only C++: no device is touched.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/msretr.h"

extern "C" int64_t msr_facet_table(const int32_t* value, int64_t n_docs, int32_t n_values, uint16_t* local, int32_t* span_off,
                                   int32_t* span_values, int32_t* value_off, int32_t* value_pos) {
    constexpr int64_t S = MSR_TERMSET_SPAN_DOCS;
    if (n_docs < 0 || n_values < 0 || (n_docs > 0 && !value)) return -1;
    const bool fill = local != nullptr;
    if (fill && (!span_off || !value_off)) return -1;
    for (int64_t d = 0; d < n_docs; ++d)
        if (value[d] < -1 || value[d] >= n_values) return -2;
    const int64_t n_spans = (n_docs + S - 1) / S;
    std::vector<int32_t> seen;
    seen.reserve((size_t)std::min<int64_t>(S, n_docs));
    int64_t T = 0;
    if (fill) span_off[0] = 0;
    for (int64_t s = 0; s < n_spans; ++s) {
        const int64_t d0 = s * S, d1 = std::min(n_docs, d0 + S);
        seen.clear();
        for (int64_t d = d0; d < d1; ++d)
            if (value[d] >= 0) seen.push_back(value[d]);
        std::sort(seen.begin(), seen.end());
        seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
        if (fill) {
            if (!seen.empty() && !span_values) return -1;
            std::copy(seen.begin(), seen.end(), span_values + T);
            for (int64_t d = d0; d < d1; ++d)
                local[d] = value[d] < 0 ? (uint16_t)0xFFFF
                                        : (uint16_t)(std::lower_bound(seen.begin(), seen.end(), value[d]) - seen.begin());
            span_off[s + 1] = (int32_t)(T + (int64_t)seen.size());
        }
        T += (int64_t)seen.size();
    }
    if (!fill) return T;
    if (T > 0 && !value_pos) return -1;
    // the transpose: slots in ascending order fall into each value's list in ascending order
    for (int64_t v = 0; v <= n_values; ++v) value_off[v] = 0;
    for (int64_t p = 0; p < T; ++p) ++value_off[span_values[p] + 1];
    for (int64_t v = 0; v < n_values; ++v) value_off[v + 1] += value_off[v];
    std::vector<int32_t> next(value_off, value_off + n_values);
    for (int64_t p = 0; p < T; ++p) value_pos[next[span_values[p]]++] = (int32_t)p;
    return T;
}
