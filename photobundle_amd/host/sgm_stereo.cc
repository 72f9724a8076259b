// sgm_stereo.cc -- see sgm_stereo.h.
#include "sgm_stereo.h"

#include <algorithm>
#include <cctype>
#include <stdexcept>

#include "utils.h"

namespace {

std::string sgmError(int rc, const pba_sgm* s) { return std::string(pba_status_string(rc)) + ": " + pba_sgm_last_error(s); }

void checked(const pba_sgm_params& p, int rows, int cols) {
  const int rc = pba_sgm_validate_params(rows, cols, &p);
  if (rc != PBA_OK) throw std::runtime_error("SgmStereo: " + sgmError(rc, nullptr));
}

}  // namespace

SgmStereo::Config::Config()
    : numberOfDisparities(128), sobelCapValue(15), censusRadius(2), windowRadius(2), smoothnessPenaltySmall(100),
      smoothnessPenaltyLarge(1600), consistencyThreshold(1), disparityFactor(256.0), censusWeightFactor(1.0 / 6.0) {}

SgmStereo::Config SgmStereo::Config::fromConfigFile(const utils::ConfigFile& cf) {
  Config c;
  c.numberOfDisparities = cf.get<int>("numberOfDisparities", c.numberOfDisparities);
  c.sobelCapValue = cf.get<int>("sobelCapValue", c.sobelCapValue);
  c.censusRadius = cf.get<int>("censusRadius", c.censusRadius);
  c.windowRadius = cf.get<int>("windowRadius", c.windowRadius);
  c.smoothnessPenaltySmall = cf.get<int>("smoothnessPenaltySmall", c.smoothnessPenaltySmall);
  c.smoothnessPenaltyLarge = cf.get<int>("smoothnessPenaltyLarge", c.smoothnessPenaltyLarge);
  c.consistencyThreshold = cf.get<int>("consistencyThreshold", c.consistencyThreshold);
  c.disparityFactor = cf.get<double>("disparityFactor", c.disparityFactor);
  c.censusWeightFactor = cf.get<double>("censusWeightFactor", c.censusWeightFactor);
  checked(c.params(), 0, 0);
  return c;
}

pba_sgm_params SgmStereo::Config::params() const {
  pba_sgm_params p;
  pba_sgm_default_params(&p);
  p.number_of_disparities = numberOfDisparities;
  p.sobel_cap_value = sobelCapValue;
  p.census_radius = censusRadius;
  p.window_radius = windowRadius;
  p.smoothness_penalty_small = smoothnessPenaltySmall;
  p.smoothness_penalty_large = smoothnessPenaltyLarge;
  p.consistency_threshold = consistencyThreshold;
  p.disparity_factor = disparityFactor;
  p.census_weight_factor = censusWeightFactor;
  return p;
}

bool SgmStereo::selectedBy(const utils::ConfigFile& cf) {
  std::string alg = cf.get<std::string>("StereoAlgorithm", "BlockMatching");
  std::transform(alg.begin(), alg.end(), alg.begin(), [](unsigned char c) { return std::tolower(c); });
  return alg == "sgm" || alg == "semiglobalmatching";
}

SgmStereo::SgmStereo(Config config, int device) : _config(config), _device(device) { checked(_config.params(), 0, 0); }

SgmStereo::~SgmStereo() { pba_sgm_destroy(_h); }

pba_sgm* SgmStereo::handle(const ImageSize& size) {
  if (_h && size.rows == _size.rows && size.cols == _size.cols) return _h;
  pba_sgm_destroy(_h);
  _h = nullptr;
  const pba_sgm_params p = _config.params();
  const int rc = pba_sgm_create(size.rows, size.cols, &p, _device, &_h);
  if (rc != PBA_OK) throw std::runtime_error("pba_sgm_create: " + sgmError(rc, nullptr));
  _size = size;
  return _h;
}

void SgmStereo::compute(const uint8_t* left, const uint8_t* right, const ImageSize& size, float* dmap) {
  pba_sgm* h = handle(size);
  const int rc = pba_sgm_compute(h, left, right, 1.0f, nullptr, dmap, nullptr);
  if (rc != PBA_OK) throw std::runtime_error("pba_sgm_compute: " + sgmError(rc, h));
}

void SgmStereo::depth(const uint8_t* left, const uint8_t* right, const ImageSize& size, float Bf, float* zmap) {
  pba_sgm* h = handle(size);
  const int rc = pba_sgm_compute(h, left, right, Bf, nullptr, nullptr, zmap);
  if (rc != PBA_OK) throw std::runtime_error("pba_sgm_compute: " + sgmError(rc, h));
}
