// item_groups.h -- which items of a batch share what: the groups of identical start fields and of identical wfe maps, the
// items whose power sums stand for others, and what a caller's same_as list may hold.  Pure host arithmetic on parameter
// records: no HIP, no context, so that a plain C++ program can test it (tests/item_groups_main.cpp).
#pragma once
#include <cstring>
#include <vector>

#pragma GCC visibility push(hidden)  // internal to the library, like everything host.h declares

// Bitwise equality of two records of `stride` doubles, index `skip` left out (-1: none; the wfe rule "same_map" skips the
// wavelength, ZP_INV_WL).  Bitwise: +0.0 and -0.0 differ, two NaNs with equal bits are equal.
inline bool same_record(const double* a, const double* b, int stride, int skip = -1) {
  if (skip < 0 || skip >= stride) return !std::memcmp(a, b, (size_t)stride * sizeof(double));
  return !std::memcmp(a, b, (size_t)skip * sizeof(double)) &&
         !std::memcmp(a + skip + 1, b + skip + 1, (size_t)(stride - skip - 1) * sizeof(double));
}

// Per item i that leads a group: members[goff[i] .. goff[i] + glen[i]) are its items, itself first, in ascending order;
// every other item has glen 0.  (doubles: the three lists go to the device through the parameter arena as they are)
struct ItemGroups {
  std::vector<double> goff, glen, members;
};

// An item that takes part joins the first earlier leader j with joins(j, i), or leads a group of its own; members are listed
// leader by leader.  Items that take no part lead nothing and are listed nowhere.
template <typename Joins, typename TakesPart>
ItemGroups group_items(int batch, Joins&& joins, TakesPart&& takes_part) {
  ItemGroups g{std::vector<double>(batch, 0.0), std::vector<double>(batch, 0.0), {}};
  std::vector<int> lead(batch, -1);
  for (int i = 0; i < batch; ++i) {
    if (!takes_part(i)) continue;
    lead[i] = i;
    for (int j = 0; j < i; ++j)
      if (lead[j] == j && joins(j, i)) { lead[i] = j; break; }
  }
  for (int i = 0; i < batch; ++i) {
    if (lead[i] != i) continue;
    g.goff[i] = (double)g.members.size();
    for (int j = i; j < batch; ++j)
      if (lead[j] == i) g.members.push_back((double)j);
    g.glen[i] = (double)g.members.size() - g.goff[i];
  }
  return g;
}

// The groups of items with one wfe map: the items whose record (`stride` doubles) is switched on (index `enable` is not 0)
// take part; two of them share if `share` and their records agree in everything but index `skip`.  The member list is never
// empty (it goes to the device as it is, and the parameter arena hands out no empty list): one 0.0 if no item takes part.
inline ItemGroups map_groups(int batch, const double* records, int stride, int enable, int skip, bool share) {
  ItemGroups g = group_items(
      batch, [&](int j, int i) { return share && same_record(records + (size_t)j * stride, records + (size_t)i * stride, stride, skip); },
      [&](int i) { return records[(size_t)i * stride + enable] != 0.0; });
  if (g.members.empty()) g.members.push_back(0.0);
  return g;
}

// lead[i] = 1 for the leaders, same[i] = the leader of item i's group (0 for an item in no group)
inline void group_leaders(const ItemGroups& g, std::vector<double>& lead, std::vector<double>& same) {
  const int batch = (int)g.goff.size();
  lead.assign(batch, 0.0);
  same.assign(batch, 0.0);
  for (int i = 0; i < batch; ++i) {
    const int g0 = (int)g.goff[i], gl = (int)g.glen[i];
    if (gl > 0) lead[i] = 1.0;
    for (int k = 0; k < gl; ++k) same[(int)g.members[g0 + k]] = (double)i;
  }
}

// Inside each group, the sub-groups of items with one wfe map: Zernike records (`stride` doubles per item) equal in
// everything but index `skip`, if `share`; the items whose record is switched off (index `enable` holds 0) form one more.
// Returns the sub-group records, three doubles each: the item whose map it is (-1: none), the offset of its members, their
// number.  g is re-pointed: goff / glen name a leader's run of sub-group records, members lists the items sub-group by
// sub-group (within one: ascending; sub-groups in the order of their first items).
inline std::vector<double> split_by_map(ItemGroups& g, const double* records, int stride, int enable, int skip, bool share) {
  const int batch = (int)g.goff.size();
  std::vector<double> subs, sub_members;
  std::vector<char> placed(batch, 0);
  for (int i = 0; i < batch; ++i) {
    const int g0 = (int)g.goff[i], gl = (int)g.glen[i];
    if (gl == 0) continue;
    const size_t first_sub = subs.size() / 3;
    for (int k = 0; k < gl; ++k) {
      const int a = (int)g.members[g0 + k];
      if (placed[a]) continue;
      const bool off = records[(size_t)a * stride + enable] == 0.0;
      subs.push_back(off ? -1.0 : (double)a);
      subs.push_back((double)sub_members.size());
      size_t count = 0;
      for (int h = k; h < gl; ++h) {
        const int b = (int)g.members[g0 + h];
        if (placed[b]) continue;
        const bool b_off = records[(size_t)b * stride + enable] == 0.0;
        if (h == k || (off && b_off) ||
            (!off && !b_off && share && same_record(records + (size_t)a * stride, records + (size_t)b * stride, stride, skip))) {
          placed[b] = 1;
          sub_members.push_back((double)b);
          ++count;
        }
      }
      subs.push_back((double)count);
    }
    g.goff[i] = (double)first_sub;
    g.glen[i] = (double)(subs.size() / 3 - first_sub);
  }
  g.members = std::move(sub_members);
  return subs;
}

// Items with identical records (`stride` doubles each) have identical power sums: power_of[i] is the first earlier item
// whose flag is set and whose record equals item i's, else i itself; compute[i] = 1 for a flagged item that stands for itself.
inline void power_representatives(int batch, const double* records, int stride, const double* flags, std::vector<double>& power_of,
                                  std::vector<double>& compute) {
  power_of.resize(batch);
  compute.resize(batch);
  for (int i = 0; i < batch; ++i) {
    int rep = i;
    for (int j = 0; j < i; ++j)
      if (flags[j] != 0.0 && same_record(records + (size_t)j * stride, records + (size_t)i * stride, stride)) { rep = j; break; }
    power_of[i] = (double)rep;
    compute[i] = (flags[i] != 0.0 && rep == i) ? 1.0 : 0.0;
  }
}

// A caller's same_as list: every entry an integer in [0, batch); self_standing: ... that names an item which names itself
inline bool same_as_valid(const double* same_as, int batch, bool self_standing) {
  for (int i = 0; i < batch; ++i) {
    const double s = same_as[i];
    if (!(s >= 0.0) || s >= (double)batch || s != (double)(int)s) return false;
    if (self_standing && same_as[(int)s] != s) return false;
  }
  return true;
}

#pragma GCC visibility pop
