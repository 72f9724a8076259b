// Stand-alone program around photobundle_amd/host/admit_lists.h (plain C++, no engine): the list merging and the visibility
// bookkeeping of Options::reobservePasses against a brute-force restatement, on hand-written and on drawn cases, fed the way the class
// feeds them from pba_admit's outputs (a capacity that cuts the candidate list short included).  Meant to be built with
// -fsanitize=address,undefined (tests/test_admit_cpu.py does); prints "ok <cases>" and returns 0, or says what differed and returns 1.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../photobundle_amd/host/admit_lists.h"

namespace {

int g_failed = 0;
void expect(bool ok, const char* what, int id) {
  if (!ok) { std::printf("case %d: %s\n", id, what); g_failed = 1; }
}

// the stand-in for the engine call: every (point, slot) pair that is not in the list, in order, cut at `capacity`; take by coin
struct Stub {
  std::vector<int32_t> cand_point, cand_slot;
  std::vector<uint8_t> cand_take;
  int n_candidates = 0, n_written = 0;
};
Stub stub_admit(const std::vector<int32_t>& op, const std::vector<int32_t>& os, int n_points, int n_slots, int capacity, std::mt19937& rng) {
  std::set<std::pair<int32_t, int32_t>> have;
  for (size_t i = 0; i < op.size(); ++i) have.insert({op[i], os[i]});
  Stub s;
  s.cand_point.resize((size_t)capacity); s.cand_slot.resize((size_t)capacity); s.cand_take.resize((size_t)capacity);
  for (int p = 0; p < n_points; ++p)
    for (int sl = 0; sl < n_slots; ++sl) {
      if (have.count({p, sl}) || rng() % 4 == 0) continue;
      if (s.n_candidates < capacity) {
        s.cand_point[(size_t)s.n_candidates] = p; s.cand_slot[(size_t)s.n_candidates] = sl; s.cand_take[(size_t)s.n_candidates] = rng() % 2;
        ++s.n_written;
      }
      ++s.n_candidates;
    }
  return s;
}

void one_case(int id, int n_points, int n_slots, int capacity, std::mt19937& rng) {
  std::vector<int32_t> op, os;
  for (int p = 0; p < n_points; ++p) {
    bool any = false;
    for (int sl = 0; sl < n_slots; ++sl)
      if (rng() % 2 || (!any && sl == n_slots - 1)) { op.push_back(p); os.push_back(sl); any = true; }
  }
  const Stub s = stub_admit(op, os, n_points, n_slots, capacity, rng);
  std::set<std::pair<int32_t, int32_t>> want;
  for (size_t i = 0; i < op.size(); ++i) want.insert({op[i], os[i]});
  int taken = 0;
  for (int c = 0; c < s.n_written; ++c)
    if (s.cand_take[(size_t)c]) { want.insert({s.cand_point[(size_t)c], s.cand_slot[(size_t)c]}); ++taken; }
  const size_t before = op.size();
  const int added = admit_lists::MergeTaken(op, os, s.n_written, s.cand_point.data(), s.cand_slot.data(), s.cand_take.data());
  expect(added == taken, "blocks added", id);
  expect(op.size() == before + (size_t)taken && os.size() == op.size() && op.size() == want.size(), "length of the merged list", id);
  size_t i = 0;
  for (const auto& w : want) {      // (a std::set of pairs iterates by point, then slot)
    if (i >= op.size()) break;
    expect(op[i] == w.first && os[i] == w.second, "merged entry", id);
    ++i;
  }
}

void visibility_cases() {
  std::vector<uint32_t> f = {3, 4, 6};
  expect(admit_lists::InsertAscending(f, 5) && f == std::vector<uint32_t>({3, 4, 5, 6}), "a frame in the middle", 1000);
  expect(admit_lists::InsertAscending(f, 7) && f.back() == 7, "the newest frame goes last", 1001);
  expect(admit_lists::InsertAscending(f, 1) && f.front() == 1, "an earlier frame goes first", 1002);
  expect(!admit_lists::InsertAscending(f, 4) && f.size() == 6, "a frame that is there stays once", 1003);
  std::vector<uint32_t> e;
  expect(admit_lists::InsertAscending(e, 9) && e == std::vector<uint32_t>({9}), "an empty list", 1004);
}

}  // namespace

int main() {
  std::mt19937 rng(12345);
  int n = 0;
  // by hand: nothing to merge; an empty candidate list with a null pointer's worth of data
  {
    std::vector<int32_t> op = {0, 0, 1}, os = {0, 2, 1};
    expect(admit_lists::MergeTaken(op, os, 0, nullptr, nullptr, nullptr) == 0 && op.size() == 3, "no candidates", n);
    ++n;
    const int32_t cp[3] = {0, 1, 1}, cs[3] = {1, 0, 2};
    const uint8_t none[3] = {0, 0, 0}, all[3] = {1, 1, 1};
    expect(admit_lists::MergeTaken(op, os, 3, cp, cs, none) == 0 && op == std::vector<int32_t>({0, 0, 1}), "nothing taken", n);
    ++n;
    expect(admit_lists::MergeTaken(op, os, 3, cp, cs, all) == 3 && op == std::vector<int32_t>({0, 0, 0, 1, 1, 1}) &&
           os == std::vector<int32_t>({0, 1, 2, 0, 1, 2}), "everything taken", n);
    ++n;
  }
  for (int n_points : {1, 2, 7, 60})
    for (int n_slots : {1, 2, 5, 32})
      for (int capacity : {0, 1, 5, n_points * n_slots}) { one_case(n, n_points, n_slots, capacity, rng); ++n; }
  visibility_cases();
  if (g_failed) return 1;
  std::printf("ok %d\n", n);
  return 0;
}
