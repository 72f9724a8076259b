// Stand-alone program around photobundle_amd/csrc/pba_mode_rules.h (plain C++, no HIP) for the rows of pba_admit.  First line: the
// number of rows and kModeAdmit (hex).  Then, for every "present on" line (feature bits in hex) of standard input: the feature
// mode_conflict names as being in the way (hex, 0 for none), a tab, the sentence ("-" for a null answer), a tab, and the sentence the
// table WITHOUT its last two rows gives (the same walk, two rows shorter).
#include <cstdio>

#include "../photobundle_amd/csrc/pba_mode_rules.h"

static const char* conflict_without_the_last_two(unsigned present, unsigned on) {
  const int n = (int)(sizeof(pba::kModeRules) / sizeof(pba::kModeRules[0])) - 2;
  for (int i = 0; i < n; ++i) {
    const pba::ModeRule& r = pba::kModeRules[i];
    const bool fwd = r.b == on && (present & r.a), bwd = r.a == on && (present & r.b);
    if (!fwd && !bwd) continue;
    return (fwd || !r.then_a) ? r.then_b : r.then_a;
  }
  return nullptr;
}

int main() {
  const int n = (int)(sizeof(pba::kModeRules) / sizeof(pba::kModeRules[0]));
  std::printf("%d\t%x\t%x %x\t%x %x\n", n, (unsigned)pba::kModeAdmit, pba::kModeRules[n - 2].a, pba::kModeRules[n - 2].b, pba::kModeRules[n - 1].a,
              pba::kModeRules[n - 1].b);
  char line[256];
  while (std::fgets(line, sizeof(line), stdin)) {
    unsigned present = 0, on = 0, with = 0;
    if (std::sscanf(line, "%x %x", &present, &on) != 2) return 2;
    const char* why = pba::mode_conflict(present, on, &with);
    const char* old = conflict_without_the_last_two(present, on);
    std::printf("%x\t%s\t%s\n", why ? with : 0u, why ? why : "-", old ? old : "-");
  }
  return 0;
}
