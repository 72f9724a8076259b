// admit_lists.h -- the host bookkeeping of Options::reobservePasses: the class's copy of the observation list merged with the candidates
// pba_admit took, and a frame id put into a visibility list that stays in ascending order.  Plain C++, no engine call: a stand-alone
// program can run it under a sanitizer (tests/admit_lists_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace admit_lists {

// obs_point / obs_slot: grouped by point, slots ascending inside a point.  cand_*: [n_cand], ordered by point then slot, disjoint from the
// list (pba_admit's output).  Afterwards the lists hold, per point, the union of the old slots and the taken ones, ascending.  Returns the
// number of blocks added.
inline int MergeTaken(std::vector<int32_t>& obs_point, std::vector<int32_t>& obs_slot, int n_cand, const int32_t* cand_point,
                      const int32_t* cand_slot, const uint8_t* cand_take) {
  std::vector<int32_t> mp, ms;
  mp.reserve(obs_point.size() + (size_t)std::max(n_cand, 0));
  ms.reserve(mp.capacity());
  size_t o = 0;
  int c = 0, added = 0;
  const auto skip = [&] { while (c < n_cand && !cand_take[c]) ++c; };
  skip();
  while (o < obs_point.size() || c < n_cand) {
    const bool old_first = o < obs_point.size() && (c >= n_cand || obs_point[o] < cand_point[c] ||
                                                    (obs_point[o] == cand_point[c] && obs_slot[o] < cand_slot[c]));
    if (old_first) { mp.push_back(obs_point[o]); ms.push_back(obs_slot[o]); ++o; }
    else { mp.push_back(cand_point[c]); ms.push_back(cand_slot[c]); ++c; ++added; skip(); }
  }
  obs_point.swap(mp);
  obs_slot.swap(ms);
  return added;
}

// f ascending: id enters at its place; false when it was there already
inline bool InsertAscending(std::vector<uint32_t>& f, uint32_t id) {
  const auto it = std::lower_bound(f.begin(), f.end(), id);
  if (it != f.end() && *it == id) return false;
  f.insert(it, id);
  return true;
}

}  // namespace admit_lists
