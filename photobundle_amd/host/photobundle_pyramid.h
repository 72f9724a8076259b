// photobundle_pyramid.h -- coarse-to-fine wrapper with the reference's interface (reference
// src/photobundle_pyramid.h:13-48).
//
// The reference implementation is unfinished (it warns "This is not finished yet", never constructs level 0, gives
// level i the calibration of level i-1 and starts its level loop out of bounds: src/photobundle_pyramid.cc:20-24,
// :40, :61).  This class implements the INTENDED behaviour:
//   * level l uses Calibration::pyrDown()^l and ImageSize::pyrDown()^l, one PhotometricBundleAdjustment per level;
//   * images: cv::pyrDown semantics (5x5 binomial [1 4 6 4 1]^2 / 256, BORDER_REFLECT_101, (sum + 128) >> 8,
//     size ((cols+1)/2, (rows+1)/2));   depth: cv::resize INTER_LINEAR semantics (the reference's call, :54-56);
//   * levels are processed coarsest -> finest; the refined frame-to-frame pose of a level initialises the next finer
//     one; the finest level's Result is returned.
#ifndef PHOTOBUNDLE_AMD_PHOTOBUNDLE_PYRAMID_H
#define PHOTOBUNDLE_AMD_PHOTOBUNDLE_PYRAMID_H

#include <vector>

#include "photobundle.h"

// cv::pyrDown for 8-bit single-channel images.
void pyrDownU8(const uint8_t* src, int rows, int cols, std::vector<uint8_t>& dst);
// cv::resize(..., INTER_LINEAR) for 32-bit float single-channel images.
void resizeBilinearF32(const float* src, int rows, int cols, int dst_rows, int dst_cols, std::vector<float>& dst);

class PhotometricBundleAdjustmentPyr {
 public:
  typedef PhotometricBundleAdjustment::Options Options;
  typedef PhotometricBundleAdjustment::Result Result;

  PhotometricBundleAdjustmentPyr(int num_levels, const Calibration& calib, const ImageSize&, const Options& = Options());
  ~PhotometricBundleAdjustmentPyr();

  void addFrame(const uint8_t* image, const float* depth_map, const Mat44& T, Result* = nullptr);

  // PhotometricBundleAdjustment::trackFrame coarse to fine: every level aligns its own image (pyrDownU8 of the finer one) to its own
  // scene points, the result of a level starts the next finer one; the finest level's result is returned.  A level with too few
  // points hands its start pose on unchanged.
  Mat44 trackFrame(const uint8_t* image, const Mat44& T_init, const TrackOptions& options = TrackOptions(), TrackResult* result = nullptr);

  int numLevels() const { return (int)_pyr.size(); }

 private:
  int _rows, _cols;
  std::vector<UniquePointer<PhotometricBundleAdjustment>> _pyr;
  std::vector<ImageSize> _sizes;
  std::vector<std::vector<uint8_t>> _im_pyr;
  std::vector<std::vector<float>> _z_pyr;
};

#endif
