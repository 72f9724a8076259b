// Test probe of the re-observation of the host class (photobundle_amd/host/photobundle.h): Options::reobservePasses and its three
// companions, Result::numAdmittedBlocks / admittedBlocks, visibilityLists(), the refusal of addFrames.  Compiled by
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

extern "C" {

// reobserve4: passes, factor, quantile, min cost; outlier_passes: Options::outlierPasses (its companions at their defaults)
int admit_probe_create(int rows, int cols, const double* K4, int window, int radius, double min_score, const double* reobserve4, int outlier_passes,
                       char* err, int errlen) {
  try {
    g_ba.reset();
    Calibration calib;
    const double c5[5] = {K4[0], K4[1], K4[2], K4[3], 0.5};
    calib.setParameters(c5);
    PhotometricBundleAdjustment::Options o;
    o.slidingWindowSize = window; o.patchRadius = radius; o.minScore = min_score; o.verbose = false;
    o.reobservePasses = (int)reobserve4[0]; o.reobserveFactor = reobserve4[1]; o.reobserveQuantile = reobserve4[2]; o.reobserveMinCost = reobserve4[3];
    o.outlierPasses = outlier_passes;
    g_ba.reset(new PhotometricBundleAdjustment(calib, ImageSize(rows, cols), o));
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrame.  ints6: an optimisation ran | poses | numAdmittedBlocks | entries of admittedBlocks | numCulledBlocks | numResiduals;
// costs2: initial, final; admitted [max_admitted][2]: (position in visibilityLists(), frame id)
int admit_probe_add(const uint8_t* image, const float* depth, const double* T16, int* ints6, double* costs2, uint32_t* admitted, int max_admitted,
                    char* err, int errlen) {
  try {
    PhotometricBundleAdjustment::Result res;
    g_ba->addFrame(image, depth, from16(T16), &res);
    ints6[0] = res.initialCost >= 0.0 ? 1 : 0;
    if (!ints6[0]) return 0;
    ints6[1] = (int)res.poses.size(); ints6[2] = res.numAdmittedBlocks; ints6[3] = (int)res.admittedBlocks.size(); ints6[4] = res.numCulledBlocks;
    ints6[5] = res.numResiduals;
    costs2[0] = res.initialCost; costs2[1] = res.finalCost;
    for (int i = 0; i < ints6[3] && i < max_admitted; ++i) { admitted[2 * i] = res.admittedBlocks[(size_t)i].first; admitted[2 * i + 1] = res.admittedBlocks[(size_t)i].second; }
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// visibilityLists(): *n_lists lists; begin [max_lists + 1] offsets into ids [max_ids].  Returns 2 when the outputs are too small
int admit_probe_visibility(int* n_lists, int* begin, int max_lists, uint32_t* ids, int max_ids, char* err, int errlen) {
  try {
    const std::vector<std::vector<uint32_t>> lists = g_ba->visibilityLists();
    *n_lists = (int)lists.size();
    if ((int)lists.size() > max_lists) return 2;
    int at = 0;
    for (size_t i = 0; i < lists.size(); ++i) {
      begin[i] = at;
      for (uint32_t id : lists[i]) { if (at >= max_ids) return 2; ids[at++] = id; }
    }
    begin[lists.size()] = at;
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// addFrames on the one instance (the refusal comes before anything is read)
int admit_probe_add_frames(const uint8_t* image, const float* depth, const double* T16, char* err, int errlen) {
  try {
    const Mat44 T = from16(T16);
    PhotometricBundleAdjustment::addFrames({g_ba.get()}, {PhotometricBundleAdjustment::Frame{image, depth, &T}}, {});
    return 0;
  } catch (const std::exception& ex) { return report(ex, err, errlen); }
}

// defaults of the new fields: out4 = Options::reobserve* (passes, factor, quantile, min cost); returns Result::numAdmittedBlocks' default
int admit_probe_defaults(double* out4) {
  const PhotometricBundleAdjustment::Options o;
  out4[0] = o.reobservePasses; out4[1] = o.reobserveFactor; out4[2] = o.reobserveQuantile; out4[3] = o.reobserveMinCost;
  PhotometricBundleAdjustment::Result r;
  return r.numAdmittedBlocks + (int)r.admittedBlocks.size();
}

// the Options a ConfigFile with the given text gives, printed as ConfigFile lines
int admit_probe_parse_and_print(const char* config_text, const char* scratch_file, char* out, int outlen, char* err, int errlen) {
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

void admit_probe_release() { g_ba.reset(); }

}  // extern "C"
