// sgm_stereo.h -- the reference's SgmStereo (reference src/stereo_algorithm.cc:95-127) on the MI355X semi-global matcher of
// include/pba_sgm.h.
//
//     SgmStereo sgm(SgmStereo::Config::fromConfigFile(cf));   // the keys and defaults of reference :229-237
//     sgm.compute(left, right, size, dmap);        // float disparity, 0 where invalid (speckle, left-right check, occlusion)
//     sgm.depth(left, right, size, Bf, zmap);      // compute + disparityToDepth fused on the device, byte-identical to the two steps
//
// StereoAlgorithm (stereo_algorithm.h) stays the block-matching wrapper; a driver that reads the StereoAlgorithm key picks
// this class for SGM / SemiGlobalMatching (SgmStereo::selectedBy).  The device handle is created at the first call for the image
// size it is given (and again when the size changes).
#ifndef PHOTOBUNDLE_AMD_SGM_STEREO_H
#define PHOTOBUNDLE_AMD_SGM_STEREO_H

#include <cstdint>
#include <string>

#include "../../include/pba_sgm.h"
#include "types.h"

namespace utils { class ConfigFile; }

class SgmStereo {
 public:
  struct Config {
    int numberOfDisparities;
    int sobelCapValue;
    int censusRadius;
    int windowRadius;
    int smoothnessPenaltySmall;
    int smoothnessPenaltyLarge;
    int consistencyThreshold;

    double disparityFactor;
    double censusWeightFactor;

    Config();
    // reads the reference's keys; throws std::runtime_error naming the key when a value is refused (no device call)
    static Config fromConfigFile(const utils::ConfigFile& cf);
    pba_sgm_params params() const;
  };

  // true when the config's StereoAlgorithm key is SGM or SemiGlobalMatching (any letter case)
  static bool selectedBy(const utils::ConfigFile& cf);

  explicit SgmStereo(Config config = Config(), int device = 0);
  ~SgmStereo();
  SgmStereo(const SgmStereo&) = delete;
  SgmStereo& operator=(const SgmStereo&) = delete;

  const Config& config() const { return _config; }

  // dmap: rows*cols floats, 0 where the disparity is invalid
  void compute(const uint8_t* left, const uint8_t* right, const ImageSize& size, float* dmap);

  // zmap: rows*cols floats of Bf / disparity, -0.1 where the disparity is <= 0.01 (imgproc.h disparityToDepth)
  void depth(const uint8_t* left, const uint8_t* right, const ImageSize& size, float Bf, float* zmap);

 private:
  pba_sgm* handle(const ImageSize& size);
  Config _config;
  int _device = 0;
  pba_sgm* _h = nullptr;
  ImageSize _size;
};

#endif
