// Test probe of the outlier culling of the host class (photobundle_amd/host/photobundle.h): Options::outlierPasses and its four
// companions, Result::numCulledBlocks / numCulledPoints, TrackOptions::outlierPasses, the refusal of addFrames.  Compiled by
// tests/host_class_probe.build() and driven through ctypes.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <fstream>
#include <memory>
#include <sstream>
#include <vector>

#include "../photobundle_amd/host/photobundle.h"
#include "../photobundle_amd/host/utils.h"

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
// outlier5: passes, quantile, factor, min cost, min observations
static PhotometricBundleAdjustment::Options options_of(int window, int radius, double min_score, const double* outlier5) {
  PhotometricBundleAdjustment::Options o;
  o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
  o.outlierPasses = (int)outlier5[0]; o.outlierQuantile = outlier5[1]; o.outlierFactor = outlier5[2]; o.outlierMinCost = outlier5[3];
  o.outlierMinObservations = (int)outlier5[4];
  return o;
}

extern "C" {

int cull_probe_create(int rows, int cols, const double* K4, int window, int radius, double min_score, const double* outlier5, char* err, int errlen) {
  try {
    g_ba.reset();
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], 0.5};
    calib.setParameters(c5);
    g_ba.reset(new PhotometricBundleAdjustment(calib, ImageSize(rows, cols), options_of(window, radius, min_score, outlier5)));
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrame.  ints6: an optimisation ran | poses | points that left | numCulledBlocks | numCulledPoints | iterations; costs2: initial, final
int cull_probe_add(const uint8_t* image, const float* depth, const double* T16, int* ints6, double* costs2, double* poses16, int max_poses,
                   char* err, int errlen) {
  try {
    PhotometricBundleAdjustment::Result res;
    g_ba->addFrame(image, depth, from16(T16), &res);
    ints6[0] = res.initialCost >= 0.0 ? 1 : 0;
    if (!ints6[0]) return 0;
    ints6[1] = (int)res.poses.size(); ints6[2] = (int)res.refinedPoints.size(); ints6[3] = res.numCulledBlocks; ints6[4] = res.numCulledPoints;
    ints6[5] = (int)res.iterationSummary.size();
    costs2[0] = res.initialCost; costs2[1] = res.finalCost;
    for (int i = 0; i < ints6[1] && i < max_poses; ++i)
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) poses16[16 * i + 4 * r + c] = res.poses[i](r, c);
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// trackFrame with TrackOptions::outlierPasses = passes; ints4: tracked | numPoints | numCulledBlocks | numCulledPoints; costs2: initial, final
int cull_probe_track(const uint8_t* image, const double* T16, int passes, double* T_out16, int* ints4, double* costs2, char* err, int errlen) {
  try {
    TrackOptions opt;
    opt.outlierPasses = passes;
    TrackResult tr;
    const Mat44 T = g_ba->trackFrame(image, from16(T16), opt, &tr);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T_out16[4 * r + c] = T(r, c);
    ints4[0] = tr.tracked ? 1 : 0; ints4[1] = tr.numPoints; ints4[2] = tr.numCulledBlocks; ints4[3] = tr.numCulledPoints;
    costs2[0] = tr.initialCost; costs2[1] = tr.finalCost;
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrames on the one instance (the refusal comes before anything is read)
int cull_probe_add_frames(const uint8_t* image, const float* depth, const double* T16, char* err, int errlen) {
  try {
    const Mat44 T = from16(T16);
    PhotometricBundleAdjustment::addFrames({g_ba.get()}, {PhotometricBundleAdjustment::Frame{image, depth, &T}}, {});
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// defaults of the new fields: out5 = Options::outlier*; returns Result / TrackOptions / TrackResult defaults as bits (0: all zero)
int cull_probe_defaults(double* out5) {
  const PhotometricBundleAdjustment::Options o;
  out5[0] = o.outlierPasses; out5[1] = o.outlierQuantile; out5[2] = o.outlierFactor; out5[3] = o.outlierMinCost; out5[4] = o.outlierMinObservations;
  PhotometricBundleAdjustment::Result r;
  TrackResult t;
  return (r.numCulledBlocks ? 1 : 0) | (r.numCulledPoints ? 2 : 0) | (TrackOptions().outlierPasses ? 4 : 0) | (t.numCulledBlocks ? 8 : 0) | (t.numCulledPoints ? 16 : 0);
}

// the Options a ConfigFile with the given text gives, printed as ConfigFile lines
int cull_probe_parse_and_print(const char* config_text, const char* scratch_file, char* out, int outlen, char* err, int errlen) {
  try {
    { std::ofstream f(scratch_file); f << config_text; }
    const utils::ConfigFile cf{std::string(scratch_file)};
    const PhotometricBundleAdjustment::Options o(cf);
    std::ostringstream os;
    os << o;
    std::snprintf(out, outlen, "%s", os.str().c_str());
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

void cull_probe_release() { g_ba.reset(); }

}  // extern "C"
