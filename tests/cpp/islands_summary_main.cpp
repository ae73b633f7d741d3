// The host half of the island census (kaboodle_amd/csrc/kb_islands_sum.h) on hand-made labels: the sizes and every
// summary field, the order of `top` past its eight entries, and the refusal of labels that no settled pass can give.
// Plain C++; tests/test_islands.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include "../../kaboodle_amd/csrc/kb_islands_sum.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  const uint32_t N = KB_CENSUS_NONE;
  {  // the 12 ids of tests/test_islands.py: 4 and 9 do not run
    const std::vector<uint32_t> label = {0, 0, 0, 3, N, 5, 3, 5, 8, N, 10, 0};
    const std::vector<uint32_t> rown = {2, 2, 2, 3, 0, 3, 2, 1, 1, 0, 2, 2};
    std::vector<uint32_t> size(12, 77);
    kb_islands s;
    CHECK(is_summary(label, rown, 7, 3, &s, size.data()));
    const uint32_t want[12] = {4, 4, 4, 2, 0, 2, 2, 2, 1, 0, 1, 4};
    for (int j = 0; j < 12; ++j) CHECK(size[j] == want[j]);
    CHECK(s.round == 7 && s.sweeps == 3 && s.observers == 10 && s.islands == 5 && s.singletons == 2 && s.rebroadcasting == 1);
    CHECK(s.largest == 4 && s.largest_label == 0 && s.second == 2 && s.unreachable_pairs == 4 * 6 + 2 * 8 + 2 * 8 + 9 + 9);
    const uint32_t top[KB_ISLANDS_TOP][2] = {{0, 4}, {3, 2}, {5, 2}, {8, 1}, {10, 1}, {N, 0}, {N, 0}, {N, 0}};
    for (int k = 0; k < KB_ISLANDS_TOP; ++k) CHECK(s.top[k][0] == top[k][0] && s.top[k][1] == top[k][1]);
    CHECK(is_summary(label, rown, 7, 3, &s, nullptr) && s.islands == 5);          // no size array asked for
  }
  {  // 11 islands: ten singletons, then one of 3 at the highest labels; top keeps the eight first in order
    std::vector<uint32_t> label(13), rown(13, 1);
    for (uint32_t j = 0; j < 10; ++j) label[j] = j;
    label[10] = label[11] = label[12] = 10;
    rown[3] = 0; rown[4] = 2;
    kb_islands s;
    CHECK(is_summary(label, rown, 0, 1, &s, nullptr));
    CHECK(s.islands == 11 && s.singletons == 10 && s.rebroadcasting == 9 && s.largest == 3 && s.largest_label == 10 && s.second == 1);
    CHECK(s.top[0][0] == 10 && s.top[0][1] == 3);
    for (uint32_t k = 1; k < KB_ISLANDS_TOP; ++k) CHECK(s.top[k][0] == k - 1 && s.top[k][1] == 1);
    CHECK(s.unreachable_pairs == 3ull * 10 + 10ull * 12);
  }
  {  // nobody runs; no ids at all
    kb_islands s;
    CHECK(is_summary({N, N, N}, {0, 0, 0}, 2, 1, &s, nullptr));
    CHECK(s.observers == 0 && s.islands == 0 && s.largest == 0 && s.largest_label == N && s.top[0][0] == N && s.unreachable_pairs == 0);
    CHECK(is_summary({}, {}, 2, 1, &s, nullptr) && s.islands == 0);
  }
  {  // labels no settled pass gives: above the id, not a root, past the capacity
    kb_islands s;
    CHECK(!is_summary({1, 1}, {1, 1}, 0, 1, &s, nullptr));
    CHECK(!is_summary({0, 0, 1}, {1, 1, 1}, 0, 1, &s, nullptr));
    CHECK(!is_summary({0, 5}, {1, 1}, 0, 1, &s, nullptr));
  }
  {  // a 64-bit sum: two islands of 70,000
    const uint32_t n = 140000;
    std::vector<uint32_t> label(n), rown(n, 5);
    for (uint32_t j = 0; j < n; ++j) label[j] = j & 1u;
    kb_islands s;
    CHECK(is_summary(label, rown, 0, 2, &s, nullptr));
    CHECK(s.unreachable_pairs == 2ull * 70000 * 70000 && s.largest == 70000 && s.largest_label == 0 && s.second == 70000);
  }
  std::printf("islands summary ok\n");
  return 0;
}
