// Stand-alone program around photobundle_amd/csrc/pba_slot_rule.h (plain C++, no HIP): reads "mask n_frames" lines (mask in hex) from
// standard input and prints, per line, the number of free slots, then is_free and free_index of every slot -- what the device's
// cam_geom_one / cam_geom_finish and the host's table sizes are computed from.  A line "@ fixed_slot" prints the mask of the old call.
#include <cstdio>

#include "../photobundle_amd/csrc/pba_slot_rule.h"

int main() {
  char line[256];
  while (std::fgets(line, sizeof(line), stdin)) {
    unsigned mask = 0;
    int n = 0;
    if (line[0] == '@') {
      if (std::sscanf(line + 1, "%d", &n) != 1) return 2;
      std::printf("%x\n", pba::slot_mask_of_fixed(n));
      continue;
    }
    if (std::sscanf(line, "%x %d", &mask, &n) != 2) return 2;
    std::printf("%d", pba::slot_count_free(mask, n));
    for (int c = 0; c < n; ++c) std::printf(" %d %d", pba::slot_is_free(mask, c), pba::slot_free_index(mask, c));
    std::printf("\n");
  }
  return 0;
}
