// Test probe of the host classes (photobundle_amd/host/photobundle.h, photobundle_pyramid.h): addFrame, trackFrame, Options::numConstantFrames
// and Options::camerasConstant.  Compiled by tests/host_class_probe.py into a temporary shared library and driven through ctypes: one
// instance of the class (levels == 1) or of the pyramid class (levels > 1).
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
static void to16(const Mat44& T, double* m) {
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = T(r, c);
}
// num_constant / cameras_constant < 0: the field keeps its default
static void set_fields(PhotometricBundleAdjustment::Options& o, int num_constant, int cameras_constant) {
  if (num_constant >= 0) o.numConstantFrames = num_constant;
  if (cameras_constant >= 0) o.camerasConstant = cameras_constant != 0;
}

extern "C" {

int probe_create(int levels, int rows, int cols, const double* K4, int window, int radius, double min_score, int num_constant,
                 int cameras_constant, char* err, int errlen) {
  try {
    g_ba.reset(); g_pyr.reset();
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], 0.5};
    calib.setParameters(c5);
    PhotometricBundleAdjustment::Options o;
    o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
    set_fields(o, num_constant, cameras_constant);
    if (levels > 1) g_pyr.reset(new PhotometricBundleAdjustmentPyr(levels, calib, ImageSize(rows, cols), o));
    else g_ba.reset(new PhotometricBundleAdjustment(calib, ImageSize(rows, cols), o));
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrame; ran = an optimisation ran; then costs3 = initial / final / fixed cost, counts2 = poses of the Result / points that left the
// window, poses16 (at most max_poses) and refined / original points (at most max_points, 3 doubles each)
int probe_add(const uint8_t* image, const float* depth, const double* T16, int* ran, double* costs3, int* counts2, double* poses16,
              int max_poses, double* refined3, double* original3, int max_points, char* err, int errlen) {
  try {
    PhotometricBundleAdjustment::Result res;
    res.initialCost = -1.0;
    if (g_pyr) g_pyr->addFrame(image, depth, from16(T16), &res);
    else g_ba->addFrame(image, depth, from16(T16), &res);
    *ran = res.initialCost >= 0.0 ? 1 : 0;
    if (*ran) {
      costs3[0] = res.initialCost; costs3[1] = res.finalCost; costs3[2] = res.fixedCost;
      counts2[0] = (int)res.poses.size(); counts2[1] = (int)res.refinedPoints.size();
      for (int i = 0; i < counts2[0] && i < max_poses; ++i) to16(res.poses[i], poses16 + 16 * i);
      for (int i = 0; i < counts2[1] && i < max_points; ++i)
        for (int k = 0; k < 3; ++k) { refined3[3 * i + k] = res.refinedPoints[i][k]; original3[3 * i + k] = res.originalPoints[i][k]; }
    }
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// trackFrame; out: refined frame-to-frame pose, tracked, numPoints, numIterations, initial / final cost, message
int probe_track(const uint8_t* image, const double* T16, int max_iterations, int min_points, double* T_out16, int* ints3, double* costs2,
                char* message, int msglen, char* err, int errlen) {
  try {
    TrackOptions opt;
    opt.maxIterations = max_iterations; opt.minPoints = min_points;
    TrackResult tr;
    const Mat44 T = g_pyr ? g_pyr->trackFrame(image, from16(T16), opt, &tr) : g_ba->trackFrame(image, from16(T16), opt, &tr);
    to16(T, T_out16);
    ints3[0] = tr.tracked ? 1 : 0; ints3[1] = tr.numPoints; ints3[2] = tr.numIterations;
    costs2[0] = tr.initialCost; costs2[1] = tr.finalCost;
    std::snprintf(message, msglen, "%s", tr.message.c_str());
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// the default arguments compile: trackFrame(image, T) alone
int probe_track_defaults(const uint8_t* image, const double* T16, double* T_out16, char* err, int errlen) {
  try {
    to16(g_pyr ? g_pyr->trackFrame(image, from16(T16)) : g_ba->trackFrame(image, from16(T16)), T_out16);
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// the default of numConstantFrames, and the settings printed as ConfigFile lines (operator<< of the options with the fields set)
int probe_default_num_constant() { return PhotometricBundleAdjustment::Options().numConstantFrames; }
int probe_print_options(int num_constant, int cameras_constant, char* out, int outlen) {
  PhotometricBundleAdjustment::Options o;
  set_fields(o, num_constant, cameras_constant);
  std::ostringstream os;
  os << o;
  std::snprintf(out, outlen, "%s", os.str().c_str());
  return 0;
}

void probe_release() { g_ba.reset(); g_pyr.reset(); }

}  // extern "C"
