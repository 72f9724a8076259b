// Test probe of the depth prior of the host class (photobundle_amd/host/photobundle.h): Options::depthPriorSigma with its ConfigFile key
// and its operator<< line, Result::depthPriorCost, the std::invalid_argument cases, and computeCovariance with one constant frame.
// Compiled by tests/host_class_probe.build() and driven through ctypes (tests/point_prior_class_probe.py).
#include <cstdint>
#include <cstdio>
#include <exception>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "../photobundle_amd/host/photobundle.h"
#include "../photobundle_amd/host/utils.h"

typedef PhotometricBundleAdjustment PBA;
static std::unique_ptr<PBA> g_ba;

static Mat44 from16(const double* m) {
  Mat44 T = Mat44::Identity();
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = m[4 * r + c];
  return T;
}

extern "C" {

// 0: an instance exists; 1: std::invalid_argument; 2: another exception (no device: pba_create).  what: the exception's text
int pp_probe_create(int rows, int cols, const double* K4, double baseline, int window, int radius, double min_score, int num_constant,
                    int compute_covariance, int marginalize, double sigma, char* what, int len) {
  g_ba.reset();
  what[0] = 0;
  try {
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], baseline};
    calib.setParameters(c5);
    calib.baseline() = baseline;      // (as run_kitti sets it)
    PBA::Options o;
    o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
    o.numConstantFrames = num_constant; o.computeCovariance = compute_covariance != 0; o.marginalize = marginalize != 0;
    o.depthPriorSigma = sigma;
    g_ba.reset(new PBA(calib, ImageSize(rows, cols), o));
    return 0;
  } catch (const std::invalid_argument& ex) {
    std::snprintf(what, len, "%s", ex.what());
    return 1;
  } catch (const std::exception& ex) {
    std::snprintf(what, len, "%s", ex.what());
    return 2;
  }
}

// addFrame.  ints4: an optimisation ran | poses | covarianceOk | free frames of the covariance; vals5: initialCost, finalCost,
// depthPriorCost, minCameraPivot, minPointPivot
int pp_probe_add(const uint8_t* image, const float* depth, const double* T16, int* ints4, double* vals5, double* poses16, int max_poses,
                 char* message, int msglen, char* err, int errlen) {
  try {
    PBA::Result res;
    g_ba->addFrame(image, depth, from16(T16), &res);
    ints4[0] = res.initialCost >= 0.0 ? 1 : 0;
    if (!ints4[0]) return 0;
    ints4[1] = (int)res.poses.size(); ints4[2] = res.covarianceOk ? 1 : 0; ints4[3] = (int)res.covarianceFrameIds.size();
    vals5[0] = res.initialCost; vals5[1] = res.finalCost; vals5[2] = res.depthPriorCost; vals5[3] = res.minCameraPivot; vals5[4] = res.minPointPivot;
    for (int i = 0; i < ints4[1] && i < max_poses; ++i)
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) poses16[16 * i + 4 * r + c] = res.poses[i](r, c);
    std::snprintf(message, msglen, "%s", res.covarianceMessage.c_str());
    return 0;
  } catch (const std::exception& ex) {
    std::snprintf(err, errlen, "%s", ex.what());
    return 1;
  }
}

// addFrames on the instance: 1 when it throws std::invalid_argument (what: its text), 0 when it does not throw, 2: another exception
int pp_probe_add_frames(int rows, int cols, char* what, int len) {
  std::vector<uint8_t> img((size_t)rows * cols, 0);
  std::vector<float> depth((size_t)rows * cols, 1.0f);
  const Mat44 T = Mat44::Identity();
  what[0] = 0;
  try {
    PBA::addFrames({g_ba.get()}, {PBA::Frame{img.data(), depth.data(), &T}}, {});
    return 0;
  } catch (const std::invalid_argument& ex) {
    std::snprintf(what, len, "%s", ex.what());
    return 1;
  } catch (const std::exception& ex) {
    std::snprintf(what, len, "%s", ex.what());
    return 2;
  }
}

// the defaults: Options::depthPriorSigma (also through an empty ConfigFile) and Result::depthPriorCost are 0
int pp_probe_defaults_are_zero() {
  utils::ConfigFile cf;
  return PBA::Options().depthPriorSigma == 0.0 && PBA::Options(cf).depthPriorSigma == 0.0 && PBA::Result().depthPriorCost == 0.0;
}
double pp_probe_config_key(const char* value) {
  utils::ConfigFile cf;
  cf("depthPriorSigma", value);
  return PBA::Options(cf).depthPriorSigma;
}
int pp_probe_print_options(double sigma, char* out, int outlen) {
  PBA::Options o;
  o.depthPriorSigma = sigma;
  std::ostringstream os;
  os << o;
  std::snprintf(out, outlen, "%s", os.str().c_str());
  return 0;
}

void pp_probe_release() { g_ba.reset(); }

}  // extern "C"
