// bbd_bn_groups.h - the call groups of a fused BatchNorm / stem launch (bbd_nn.hip) as the caller described them.  Plain
// C++ with no HIP in it, shared with the stand-alone walk under the sanitizers (tests/sanitize/bn_groups_main.cpp).
#pragma once
#include <stdint.h>

#include "../../include/bbd_hip.h"

// Exactly one table: `host_rows` = prefix sums rows[0..G] in host memory, the last `untracked` groups leave the running
// statistics alone; or `dev_table` = the device table of bbd_bn_act_grouped_dev_*, which the host cannot read: `bound` is
// the caller's word for its largest group.
struct BbdBnGroups { const int32_t* host_rows; const int32_t* dev_table; int G; int untracked; int bound; };

// Validates `g` against a batch of N rows and writes G, untracked and rows[] or rows_dev into the launch arguments (BnArgs,
// or anything with those fields); returns the largest group, 0 = refuse (`a` is then not to be used).
template <class Args>
inline int bbd_bn_resolve_groups(const BbdBnGroups& g, int N, Args* a) {
  if ((g.host_rows == nullptr) == (g.dev_table == nullptr) || g.G < 1 || g.G > BBD_BN_MAX_GROUPS) return 0;
  a->G = g.G;
  if (g.dev_table) {
    a->rows_dev = g.dev_table;
    return g.bound >= 1 && g.bound <= N ? g.bound : 0;
  }
  if (g.host_rows[0] != 0 || g.host_rows[g.G] != N || g.untracked < 0 || g.untracked >= g.G) return 0;
  int biggest = 0;
  for (int i = 0; i < g.G; ++i) {
    const int n = g.host_rows[i + 1] - g.host_rows[i];
    if (n <= 0) return 0;
    biggest = n > biggest ? n : biggest;
  }
  a->untracked = g.untracked;
  for (int i = 0; i <= g.G; ++i) a->rows[i] = g.host_rows[i];
  return biggest;
}
