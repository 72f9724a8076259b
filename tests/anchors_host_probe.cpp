// Test probe of Options::numConstantFrames (photobundle_amd/host/photobundle.h), compiled by tests/anchors_probe.py into a temporary
// shared library and driven through ctypes: one instance of the class (levels == 1) or of the pyramid class (levels > 1).
#include <cstdint>
#include <cstdio>
#include <exception>
#include <memory>
#include <sstream>

#include "../photobundle_amd/host/photobundle.h"
#include "../photobundle_amd/host/photobundle_pyramid.h"

static std::unique_ptr<PhotometricBundleAdjustment> g_ba;
static std::unique_ptr<PhotometricBundleAdjustmentPyr> g_pyr;

static int report(const std::exception& ex, char* err, int errlen) {
  std::snprintf(err, errlen, "%s", ex.what());
  return 1;
}
static Mat44 from16(const double* m) {
  Mat44 T = Mat44::Identity();
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = m[4 * r + c];
  return T;
}

extern "C" {

// num_constant < 0: the field keeps its default
int probe_anchors_create(int levels, int rows, int cols, const double* K4, int window, int radius, double min_score, int num_constant,
                         char* err, int errlen) {
  try {
    g_ba.reset(); g_pyr.reset();
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], 0.5};
    calib.setParameters(c5);
    PhotometricBundleAdjustment::Options o;
    o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
    if (num_constant >= 0) o.numConstantFrames = num_constant;
    if (levels > 1) g_pyr.reset(new PhotometricBundleAdjustmentPyr(levels, calib, ImageSize(rows, cols), o));
    else g_ba.reset(new PhotometricBundleAdjustment(calib, ImageSize(rows, cols), o));
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrame; *n_poses = poses of the Result when an optimisation ran (written to poses16, at most max_poses), else 0
int probe_anchors_add(const uint8_t* image, const float* depth, const double* T16, double* poses16, int max_poses, int* n_poses,
                      double* fixed_cost, char* err, int errlen) {
  try {
    PhotometricBundleAdjustment::Result res;
    res.initialCost = -1.0;
    if (g_pyr) g_pyr->addFrame(image, depth, from16(T16), &res);
    else g_ba->addFrame(image, depth, from16(T16), &res);
    *n_poses = 0;
    if (res.initialCost >= 0.0) {
      *n_poses = (int)res.poses.size();
      *fixed_cost = res.fixedCost;
      for (int i = 0; i < *n_poses && i < max_poses; ++i)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) poses16[16 * i + 4 * r + c] = res.poses[i](r, c);
    }
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// the default of the field, and the settings printed as ConfigFile lines
int probe_anchors_default() { return PhotometricBundleAdjustment::Options().numConstantFrames; }
int probe_anchors_print_options(int num_constant, char* out, int outlen) {
  PhotometricBundleAdjustment::Options o;
  o.numConstantFrames = num_constant;
  std::ostringstream os;
  os << o;
  std::snprintf(out, outlen, "%s", os.str().c_str());
  return 0;
}

void probe_anchors_release() { g_ba.reset(); g_pyr.reset(); }

}  // extern "C"
