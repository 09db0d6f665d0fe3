// Stand-alone walk of the call-group resolution of the fused BatchNorm / stem entry points
// (baseboostdepth_amd/csrc/bbd_bn_groups.h: what every bbd_bn_act_* and bbd_stem_* call does with its group arguments
// before it launches), with nothing of the GPU:
//
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -std=c++17 \
//       tests/sanitize/bn_groups_main.cpp -o bn_groups_main && ./bn_groups_main
//
// Host tables are heap allocations of exactly G + 1 entries, so a read past a table is a sanitizer report; the launch
// arguments are a struct with the fields of BnArgs the resolution writes, between two guards.  Accepted tables must come
// back with the largest group and the fields filled, refused ones with 0.  Nothing here is loaded into Python.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../baseboostdepth_amd/csrc/bbd_bn_groups.h"

static int failures = 0;
#define CHECK(cond, ...)                                                    \
  do {                                                                      \
    if (!(cond)) {                                                          \
      failures++; fprintf(stderr, "FAIL %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); \
    }                                                                       \
  } while (0)

struct Args {
  int guard0;
  int G, untracked;
  const int32_t* rows_dev;
  int rows[BBD_BN_MAX_GROUPS + 1];
  int guard1;
};

static std::vector<int32_t> prefix(const std::vector<int>& sizes) {
  std::vector<int32_t> rows(sizes.size() + 1, 0);
  for (size_t i = 0; i < sizes.size(); ++i) rows[i + 1] = rows[i] + sizes[i];
  return rows;
}

// a host table of `sizes` handed in as G groups with `untracked` padding groups for a batch of N rows
static int host(const char* what, const std::vector<int>& sizes, int G, int untracked, int N, int want) {
  const std::vector<int32_t> rows = prefix(sizes);
  Args a;
  memset(&a, 0, sizeof a);
  a.guard0 = a.guard1 = 0x5a5a5a5a;
  const BbdBnGroups g = {rows.data(), nullptr, G, untracked, 0};
  const int got = bbd_bn_resolve_groups(g, N, &a);
  CHECK(got == want, "%s: largest group %d, expected %d", what, got, want);
  CHECK(a.guard0 == 0x5a5a5a5a && a.guard1 == 0x5a5a5a5a, "%s: wrote outside the group fields", what);
  if (got) {
    CHECK(a.G == G && a.untracked == untracked && a.rows_dev == nullptr, "%s: G %d untracked %d", what, a.G, a.untracked);
    for (int i = 0; i <= G; ++i) CHECK(a.rows[i] == rows[(size_t)i], "%s: rows[%d] = %d", what, i, a.rows[i]);
  }
  return got;
}

static int device(const char* what, const int32_t* table, int G, int bound, int N, int want) {
  Args a;
  memset(&a, 0, sizeof a);
  a.guard0 = a.guard1 = 0x5a5a5a5a;
  const BbdBnGroups g = {nullptr, table, G, 0, bound};
  const int got = bbd_bn_resolve_groups(g, N, &a);
  CHECK(got == want, "%s: largest group %d, expected %d", what, got, want);
  CHECK(a.guard0 == 0x5a5a5a5a && a.guard1 == 0x5a5a5a5a, "%s: wrote outside the group fields", what);
  if (got) {
    CHECK(a.G == G && a.untracked == 0 && a.rows_dev == table, "%s: G %d", what, a.G);
    for (int i = 0; i <= BBD_BN_MAX_GROUPS; ++i) CHECK(a.rows[i] == 0, "%s: rows[%d] written", what, i);
  }
  return got;
}

int main() {
  const int MAXG = BBD_BN_MAX_GROUPS;
  // accepted
  host("one group", {5}, 1, 0, 5, 5);
  host("three groups, one of them padding", {2, 1, 2}, 3, 1, 5, 2);
  host("32 groups", std::vector<int>(MAXG, 3), MAXG, MAXG - 1, 3 * MAXG, 3);
  std::vector<int> uneven(MAXG, 1);
  uneven[MAXG - 1] = 9;
  host("32 groups, the last one largest", uneven, MAXG, 0, MAXG + 8, 9);
  // refused (the table of 33 groups exists in full: the refusal must not depend on reading past a shorter one)
  host("33 groups", std::vector<int>(MAXG + 1, 1), MAXG + 1, 0, MAXG + 1, 0);
  host("no groups", {5}, 0, 0, 5, 0);
  host("rows[G] != N", {2, 3}, 2, 0, 6, 0);
  host("rows[G] != N, first G of a longer table", {2, 3, 1}, 2, 0, 6 + 1, 0);
  host("an empty group", {2, 0, 3}, 3, 0, 5, 0);
  host("a negative group", {4, -1, 2}, 3, 0, 5, 0);
  host("untracked = G", {2, 3}, 2, 2, 5, 0);
  host("untracked < 0", {2, 3}, 2, -1, 5, 0);
  {
    Args a;
    memset(&a, 0, sizeof a);
    const BbdBnGroups none = {nullptr, nullptr, 1, 0, 1};
    CHECK(bbd_bn_resolve_groups(none, 5, &a) == 0, "NULL tables");
    const int32_t rows[2] = {0, 5};
    const BbdBnGroups both = {rows, rows, 1, 0, 5};
    CHECK(bbd_bn_resolve_groups(both, 5, &a) == 0, "two tables");
  }
  // the device table is never read on the host: an address that is no host memory at all
  const int32_t* table = reinterpret_cast<const int32_t*>(static_cast<uintptr_t>(0x10000));
  device("device table, G = 1", table, 1, 5, 5, 5);
  device("device table, G = 32", table, MAXG, 2, 5, 2);
  device("device table, G = 33", table, MAXG + 1, 2, 5, 0);
  device("device table, G = 0", table, 0, 2, 5, 0);
  device("device bound 0", table, 8, 0, 5, 0);
  device("device bound N + 1", table, 8, 6, 5, 0);
  printf("bn call groups: %s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
