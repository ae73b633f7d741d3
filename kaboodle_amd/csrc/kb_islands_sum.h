// kb_islands_sum.h — the host half of the island census (include/kaboodle_islands.h): the islands'
// sizes as a histogram of the settled labels, and the summary's O(ids) reductions.  Plain C++ with no HIP in it, so
// it also compiles into a stand-alone host program; kb_islands.h includes it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "../../include/kaboodle_islands.h"

// label: [C] the settled labels, KB_CENSUS_NONE where the id does not run.  rown: [C] the entries of each running
// row (ids < C).  size (may be null): [C], filled.  A label that is no running id's own (label[label[j]] != label[j],
// or a label >= C) cannot come out of a settled pass; false says so and leaves *out zeroed.
static bool is_summary(const std::vector<uint32_t>& label, const std::vector<uint32_t>& rown, int32_t round,
                       uint32_t sweeps, kb_islands* out, uint32_t* size) {
  const size_t C = label.size();
  memset(out, 0, sizeof *out);
  out->round = round; out->sweeps = sweeps; out->largest_label = KB_CENSUS_NONE;
  for (uint32_t k = 0; k < KB_ISLANDS_TOP; ++k) { out->top[k][0] = KB_CENSUS_NONE; out->top[k][1] = 0; }
  std::vector<uint32_t> hist(C, 0);
  for (size_t j = 0; j < C; ++j) {
    const uint32_t lb = label[j];
    if (lb == KB_CENSUS_NONE) continue;
    if (lb > j || label[lb] != lb) return false;
    ++hist[lb]; ++out->observers;
  }
  std::vector<std::pair<uint32_t, uint32_t>> best;   // (size, label) of the KB_ISLANDS_TOP first islands so far, in order
  for (size_t j = 0; j < C; ++j) {
    const uint32_t lb = label[j], n = lb == KB_CENSUS_NONE ? 0u : hist[lb];
    if (size) size[j] = n;
    if (lb != j) continue;                            // one visit per island, at its label, labels ascending
    ++out->islands;
    out->unreachable_pairs += (uint64_t)n * (out->observers - n);
    if (n == 1) { ++out->singletons; out->rebroadcasting += rown[j] <= 1; }
    // size descending, label ascending: a later island goes behind every island that is not smaller
    auto at = std::find_if(best.begin(), best.end(), [&](const std::pair<uint32_t, uint32_t>& b) { return b.first < n; });
    if (at - best.begin() < KB_ISLANDS_TOP) {
      best.insert(at, std::make_pair(n, (uint32_t)j));
      if (best.size() > KB_ISLANDS_TOP) best.pop_back();
    }
  }
  for (size_t k = 0; k < best.size(); ++k) { out->top[k][0] = best[k].second; out->top[k][1] = best[k].first; }
  if (!best.empty()) { out->largest = best[0].first; out->largest_label = best[0].second; }
  if (best.size() > 1) out->second = best[1].first;
  return true;
}
