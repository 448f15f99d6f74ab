// host/chunk_plan.hpp from a plain C++ program (no HIP): one unit size per
// input row "rule cus count bytes lanes_per_cu floor odd", the rules called as
// the dispatch calls them (tests/test_chunk_plan.py).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "host/chunk_plan.hpp"

using namespace rure_amd;

int main() {
  char rule[32];
  uint64_t cus, count, bytes, per_cu, floor;
  int odd;
  while (scanf("%31s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d", rule, &cus, &count, &bytes,
               &per_cu, &floor, &odd) == 7) {
    const uint64_t lanes = cus * per_cu;
    uint64_t c;
    if (!strcmp(rule, "long")) c = unit_bytes(bytes, count, lanes, kLongFloor);
    else if (!strcmp(rule, "split")) c = split_unit_bytes(bytes, count, cus);
    else if (!strcmp(rule, "suffix")) c = unit_bytes(bytes, count, cus * kLanesPerCu, kLongFloor);
    else if (!strcmp(rule, "suffix_forced")) c = unit_bytes(bytes, count, cus * kLanesPerCu, kLineFloor);
    else if (!strcmp(rule, "iter")) c = unit_bytes(bytes, count, lanes, kIterFloor);
    else if (!strcmp(rule, "ragged")) c = unit_bytes(bytes, 1, lanes, kIterFloor, true, Share::RoundDown);
    else if (!strcmp(rule, "device")) c = unit_bytes(bytes, 1, lanes, floor, odd != 0);
    else if (!strcmp(rule, "odd_lines")) c = odd_lines(bytes);
    else return 2;
    printf("%" PRIu64 "\n", c);
  }
  printf("long_span %" PRIu64 " lanes_per_cu %" PRIu64 "\n", kLongSpan, kLanesPerCu);
  return 0;
}
