// stereo_algorithm.h -- the reference's StereoAlgorithm (reference src/stereo_algorithm.h:14-36) for the one algorithm its
// shipped config selects, BlockMatching, on the MI355X matcher of include/pba_stereo.h.
//
//     StereoAlgorithm stereo(cf);                 // same keys and defaults as reference src/stereo_algorithm.cc:208, :246-264
//     stereo.run(left, right, size, dmap);        // float disparity = int16 output / 16 (the reference's convertTo(1/16))
//     stereo.depth(left, right, size, Bf, zmap);  // run + disparityToDepth fused on the device, byte-identical to the two steps
//
// SGBM, SGM and RSGM (reference :210-245) are not built and throw.  The device handle is created at the first call for the
// image size it is given (and again when the size changes).
#ifndef PHOTOBUNDLE_AMD_STEREO_ALGORITHM_H
#define PHOTOBUNDLE_AMD_STEREO_ALGORITHM_H

#include <cstdint>
#include <string>

#include "../../include/pba_stereo.h"
#include "types.h"

namespace utils { class ConfigFile; }

class StereoAlgorithm {
 public:
  explicit StereoAlgorithm(const utils::ConfigFile& cf, int device = 0);
  explicit StereoAlgorithm(const std::string& conf_fn, int device = 0);
  ~StereoAlgorithm();
  StereoAlgorithm(const StereoAlgorithm&) = delete;
  StereoAlgorithm& operator=(const StereoAlgorithm&) = delete;

  // dmap: rows*cols floats, FILTERED pixels at getInvalidValue()
  void run(const uint8_t* left, const uint8_t* right, const ImageSize& size, float* dmap);
  void run(const Image_<uint8_t>& left, const Image_<uint8_t>& right, float* dmap);

  // zmap: rows*cols floats of Bf / disparity, -0.1 where the disparity is <= 0.01 (imgproc.h disparityToDepth)
  void depth(const uint8_t* left, const uint8_t* right, const ImageSize& size, float Bf, float* zmap);

  // minDisparity - 1: the float disparity of a FILTERED pixel.  (The reference returns (minDisparity - 1) / 16, which is not a
  // value its own run() produces: DESIGN.md "Stereo block matching".)
  float getInvalidValue() const;

  const pba_stereo_bm_params& params() const { return _p; }

 private:
  pba_stereo* handle(const ImageSize& size);
  pba_stereo_bm_params _p;
  int _device = 0;
  pba_stereo* _h = nullptr;
  ImageSize _size;
};

#endif
