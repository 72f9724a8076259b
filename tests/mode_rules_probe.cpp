// Stand-alone program around photobundle_amd/csrc/pba_mode_rules.h (plain C++, no HIP): reads "present on" lines (feature bits in hex)
// from standard input and prints, per line, the feature mode_conflict names as being in the way (hex, 0 for none), a tab, and the
// sentence ("-" for a null answer).
#include <cstdio>

#include "../photobundle_amd/csrc/pba_mode_rules.h"

int main() {
  char line[256];
  while (std::fgets(line, sizeof(line), stdin)) {
    unsigned present = 0, on = 0, with = 0;
    if (std::sscanf(line, "%x %x", &present, &on) != 2) return 2;
    const char* why = pba::mode_conflict(present, on, &with);
    if (why != pba::mode_conflict(present, on)) return 3;      // (the answer does not depend on asking for `with`)
    std::printf("%x\t%s\n", why ? with : 0u, why ? why : "-");
  }
  return 0;
}
