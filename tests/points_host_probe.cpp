// Test probe of Options::camerasConstant (photobundle_amd/host/photobundle.h), compiled by tests/points_probe.py into a temporary shared
// library and driven through ctypes: one instance of the host class whose optimisations hold every camera constant (or not).
#include <cstdint>
#include <cstdio>
#include <exception>
#include <memory>
#include <sstream>

#include "../photobundle_amd/host/photobundle.h"

static std::unique_ptr<PhotometricBundleAdjustment> g_ba;

static int report(const std::exception& ex, char* err, int errlen) {
  std::snprintf(err, errlen, "%s", ex.what());
  return 1;
}

extern "C" {

int probe_points_create(int rows, int cols, const double* K4, int window, int radius, double min_score, int cameras_constant, char* err, int errlen) {
  try {
    g_ba.reset();
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], 0.5};
    calib.setParameters(c5);
    PhotometricBundleAdjustment::Options o;
    o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
    o.camerasConstant = cameras_constant != 0;
    g_ba.reset(new PhotometricBundleAdjustment(calib, ImageSize(rows, cols), o));
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrame; ran = an optimisation ran; then costs2 = initial / final cost, counts2 = poses / points that left the window, poses16
// (at most max_poses) and refined / original points (at most max_points, 3 doubles each)
int probe_points_add(const uint8_t* image, const float* depth, const double* T16, int* ran, double* costs2, int* counts2, double* poses16,
                     int max_poses, double* refined3, double* original3, int max_points, char* err, int errlen) {
  try {
    Mat44 T = Mat44::Identity();
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = T16[4 * r + c];
    PhotometricBundleAdjustment::Result res;
    res.initialCost = -1.0;
    g_ba->addFrame(image, depth, T, &res);
    *ran = res.initialCost >= 0.0 ? 1 : 0;
    if (*ran) {
      costs2[0] = res.initialCost; costs2[1] = res.finalCost;
      counts2[0] = (int)res.poses.size(); counts2[1] = (int)res.refinedPoints.size();
      for (int i = 0; i < counts2[0] && i < max_poses; ++i)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) poses16[16 * i + 4 * r + c] = res.poses[i](r, c);
      for (int i = 0; i < counts2[1] && i < max_points; ++i)
        for (int k = 0; k < 3; ++k) { refined3[3 * i + k] = res.refinedPoints[i][k]; original3[3 * i + k] = res.originalPoints[i][k]; }
    }
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// operator<< of the options with the field set: what a ConfigFile would read back
int probe_points_print_options(int cameras_constant, char* out, int outlen) {
  PhotometricBundleAdjustment::Options o;
  o.camerasConstant = cameras_constant != 0;
  std::ostringstream os;
  os << o;
  std::snprintf(out, outlen, "%s", os.str().c_str());
  return 0;
}

void probe_points_release() { g_ba.reset(); }

}  // extern "C"
