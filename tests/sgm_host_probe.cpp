// Test probe of the host semi-global surface (photobundle_amd/host/sgm_stereo.h), compiled by tests/test_sgm_cpu.py and
// tests/test_gpu_sgm.py into a temporary shared library and driven through ctypes.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <memory>

#include "../photobundle_amd/host/sgm_stereo.h"
#include "../photobundle_amd/host/utils.h"

static std::unique_ptr<SgmStereo> g_sgm;

static int report(const std::exception& ex, char* err, int errlen) {
  std::snprintf(err, errlen, "%s", ex.what());
  return 1;
}

extern "C" {

// SgmStereo::Config::fromConfigFile(cfg_path) -> 7 ints and 2 doubles in Config's order, and whether the StereoAlgorithm key selects
// the semi-global matcher; 1 + message on throw.  On success the probe holds an SgmStereo of that config.
int probe_sgm_parse(const char* cfg_path, int32_t* ints, double* doubles, int32_t* selected, char* err, int errlen) {
  try {
    const utils::ConfigFile cf(cfg_path);
    *selected = SgmStereo::selectedBy(cf) ? 1 : 0;
    const SgmStereo::Config c = SgmStereo::Config::fromConfigFile(cf);
    const int32_t v[7] = {c.numberOfDisparities, c.sobelCapValue, c.censusRadius, c.windowRadius, c.smoothnessPenaltySmall,
                          c.smoothnessPenaltyLarge, c.consistencyThreshold};
    for (int i = 0; i < 7; ++i) ints[i] = v[i];
    doubles[0] = c.disparityFactor;
    doubles[1] = c.censusWeightFactor;
    g_sgm.reset(new SgmStereo(c));
    return 0;
  } catch (const std::exception& ex) {
    g_sgm.reset();
    return report(ex, err, errlen);
  }
}

int probe_sgm_compute(const uint8_t* left, const uint8_t* right, int rows, int cols, float* dmap, char* err, int errlen) {
  try {
    g_sgm->compute(left, right, ImageSize(rows, cols), dmap);
    return 0;
  } catch (const std::exception& ex) {
    return report(ex, err, errlen);
  }
}

int probe_sgm_depth(const uint8_t* left, const uint8_t* right, int rows, int cols, float bf, float* zmap, char* err, int errlen) {
  try {
    g_sgm->depth(left, right, ImageSize(rows, cols), bf, zmap);
    return 0;
  } catch (const std::exception& ex) {
    return report(ex, err, errlen);
  }
}

void probe_sgm_release() { g_sgm.reset(); }

}  // extern "C"
