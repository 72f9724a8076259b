// Test probe of the host stereo surface (photobundle_amd/host/stereo_algorithm.h, imgproc.h disparityToDepth), compiled by
// tests/test_stereo_bm_cpu.py and tests/test_gpu_stereo.py into a temporary shared library and driven through ctypes.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>

#include "../photobundle_amd/host/imgproc.h"
#include "../photobundle_amd/host/stereo_algorithm.h"
#include "../photobundle_amd/host/utils.h"

static std::unique_ptr<StereoAlgorithm> g_alg;

static int report(const std::exception& ex, char* err, int errlen) {
  std::snprintf(err, errlen, "%s", ex.what());
  return 1;
}

extern "C" {

// parses cfg_path into a StereoAlgorithm: params (12 int32, pba_stereo_bm_params order) and getInvalidValue(); 1 + message on throw
int probe_parse(const char* cfg_path, int32_t* params, float* invalid, char* err, int errlen) {
  try {
    g_alg.reset(new StereoAlgorithm(utils::ConfigFile(cfg_path)));
    std::memcpy(params, &g_alg->params(), sizeof(pba_stereo_bm_params));
    *invalid = g_alg->getInvalidValue();
    return 0;
  } catch (const std::exception& ex) {
    g_alg.reset();
    return report(ex, err, errlen);
  }
}

// run() and depth() of the StereoAlgorithm of the last successful probe_parse
int probe_run(const uint8_t* left, const uint8_t* right, int rows, int cols, float* dmap, char* err, int errlen) {
  try {
    g_alg->run(left, right, ImageSize(rows, cols), dmap);
    return 0;
  } catch (const std::exception& ex) {
    return report(ex, err, errlen);
  }
}

int probe_depth(const uint8_t* left, const uint8_t* right, int rows, int cols, float bf, float* zmap, char* err, int errlen) {
  try {
    g_alg->depth(left, right, ImageSize(rows, cols), bf, zmap);
    return 0;
  } catch (const std::exception& ex) {
    return report(ex, err, errlen);
  }
}

void probe_release() { g_alg.reset(); }

void probe_disparity_to_depth(const float* dmap, int rows, int cols, float bf, float* zmap) {
  disparityToDepth(dmap, ImageSize(rows, cols), bf, zmap);
}

}  // extern "C"
