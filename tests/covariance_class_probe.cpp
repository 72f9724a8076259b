// Test probe of the covariance output of the host class (photobundle_amd/host/photobundle.h): Options::computeCovariance, the Result
// fields it fills, TrackOptions::computeCovariance.  Compiled by tests/host_class_probe.build() and driven through ctypes.
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
static Mat44 from16(const double* m) {
  Mat44 T = Mat44::Identity();
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T(r, c) = m[4 * r + c];
  return T;
}

extern "C" {

int cov_probe_create(int rows, int cols, const double* K4, int window, int radius, double min_score, int num_constant, int cameras_constant,
                     int compute_covariance, char* err, int errlen) {
  try {
    g_ba.reset();
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], 0.5};
    calib.setParameters(c5);
    PhotometricBundleAdjustment::Options o;
    o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
    o.numConstantFrames = num_constant; o.camerasConstant = cameras_constant != 0; o.computeCovariance = compute_covariance != 0;
    g_ba.reset(new PhotometricBundleAdjustment(calib, ImageSize(rows, cols), o));
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrame.  ints5: an optimisation ran | poses | points that left the window | covarianceOk | free frames of the covariance;
// pivots2: minCameraPivot, minPointPivot; frame_ids (at most 32); pose_cov (at most 192 x 192); point_cov9 (at most max_points)
int cov_probe_add(const uint8_t* image, const float* depth, const double* T16, int* ints5, double* poses16, int max_poses, double* refined3,
                  int max_points, double* pivots2, int* frame_ids, double* pose_cov, double* point_cov9, int* n_point_cov, char* message,
                  int msglen, char* err, int errlen) {
  try {
    PhotometricBundleAdjustment::Result res;
    g_ba->addFrame(image, depth, from16(T16), &res);
    ints5[0] = res.initialCost >= 0.0 ? 1 : 0;
    if (!ints5[0]) return 0;
    ints5[1] = (int)res.poses.size(); ints5[2] = (int)res.refinedPoints.size(); ints5[3] = res.covarianceOk ? 1 : 0;
    ints5[4] = (int)res.covarianceFrameIds.size();
    for (int i = 0; i < ints5[1] && i < max_poses; ++i)
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) poses16[16 * i + 4 * r + c] = res.poses[i](r, c);
    for (int i = 0; i < ints5[2] && i < max_points; ++i) for (int k = 0; k < 3; ++k) refined3[3 * i + k] = res.refinedPoints[i][k];
    pivots2[0] = res.minCameraPivot; pivots2[1] = res.minPointPivot;
    for (int i = 0; i < ints5[4] && i < 32; ++i) frame_ids[i] = (int)res.covarianceFrameIds[i];
    for (size_t i = 0; i < res.poseCovariance.size() && i < (size_t)192 * 192; ++i) pose_cov[i] = res.poseCovariance[i];
    if (res.poseCovariance.size() != (size_t)36 * ints5[4] * ints5[4]) throw std::runtime_error("poseCovariance is not n x n");
    *n_point_cov = (int)res.refinedPointCovariances.size();
    for (int i = 0; i < *n_point_cov && i < max_points; ++i)
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) point_cov9[9 * i + 3 * r + c] = res.refinedPointCovariances[i](r, c);
    std::snprintf(message, msglen, "%s", res.covarianceMessage.c_str());
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// trackFrame with TrackOptions::computeCovariance = compute; out: pose, tracked | covarianceOk, covariance (36), minPivot
int cov_probe_track(const uint8_t* image, const double* T16, int compute, double* T_out16, int* ints2, double* cov36, double* min_pivot,
                    char* err, int errlen) {
  try {
    TrackOptions opt;
    opt.computeCovariance = compute != 0;
    TrackResult tr;
    const Mat44 T = g_ba->trackFrame(image, from16(T16), opt, &tr);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T_out16[4 * r + c] = T(r, c);
    ints2[0] = tr.tracked ? 1 : 0; ints2[1] = tr.covarianceOk ? 1 : 0;
    for (int i = 0; i < 36; ++i) cov36[i] = tr.covariance[i];
    *min_pivot = tr.minPivot;
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// defaults of the new fields: Options::computeCovariance, TrackOptions::computeCovariance, Result::covarianceOk, TrackResult::covarianceOk
int cov_probe_defaults() {
  PhotometricBundleAdjustment::Result r;
  return (PhotometricBundleAdjustment::Options().computeCovariance ? 1 : 0) | (TrackOptions().computeCovariance ? 2 : 0) |
         (r.covarianceOk ? 4 : 0) | (TrackResult().covarianceOk ? 8 : 0) |
         (r.covarianceFrameIds.empty() && r.poseCovariance.empty() && r.refinedPointCovariances.empty() && r.covarianceMessage.empty() ? 0 : 16);
}
int cov_probe_print_options(int compute_covariance, char* out, int outlen) {
  PhotometricBundleAdjustment::Options o;
  o.computeCovariance = compute_covariance != 0;
  std::ostringstream os;
  os << o;
  std::snprintf(out, outlen, "%s", os.str().c_str());
  return 0;
}

void cov_probe_release() { g_ba.reset(); }

}  // extern "C"
