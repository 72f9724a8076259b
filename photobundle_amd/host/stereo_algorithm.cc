// stereo_algorithm.cc -- see stereo_algorithm.h.
#include "stereo_algorithm.h"

#include <algorithm>
#include <cctype>
#include <stdexcept>
#include <vector>

#include "utils.h"

namespace {

std::string lower(std::string s) {
  std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return std::tolower(c); });
  return s;
}

std::string stereoError(int rc, const pba_stereo* s) {
  return std::string(pba_status_string(rc)) + ": " + pba_stereo_last_error(s);
}

}  // namespace

StereoAlgorithm::StereoAlgorithm(const std::string& conf_fn, int device) : StereoAlgorithm(utils::ConfigFile(conf_fn), device) {}

StereoAlgorithm::StereoAlgorithm(const utils::ConfigFile& cf, int device) : _device(device) {
  const std::string alg = lower(cf.get<std::string>("StereoAlgorithm", "BlockMatching"));
  if (alg == "sgbm" || alg == "semiglobalblockmatching" || alg == "sgm" || alg == "semiglobalmatching" || alg == "rsgm")
    throw std::runtime_error("StereoAlgorithm " + cf.get<std::string>("StereoAlgorithm") +
                             " is not supported: only BlockMatching (BM) is built");
  if (alg != "blockmatching" && alg != "bm") throw std::runtime_error("Unknown stereo algorithm " + cf.get<std::string>("StereoAlgorithm"));
  pba_stereo_default_params(&_p);
  _p.pre_filter_type = cf.get<int>("preFilterType", _p.pre_filter_type);
  _p.pre_filter_size = cf.get<int>("preFilterSize", _p.pre_filter_size);
  _p.pre_filter_cap = cf.get<int>("preFilterCap", _p.pre_filter_cap);
  _p.sad_window_size = cf.get<int>("SADWindowSize", _p.sad_window_size);
  _p.min_disparity = cf.get<int>("minDisparity", _p.min_disparity);
  _p.number_of_disparities = cf.get<int>("numberOfDisparities");   // must be provided (reference :258)
  _p.texture_threshold = cf.get<int>("textureThreshold", _p.texture_threshold);
  _p.uniqueness_ratio = cf.get<int>("uniquenessRatio", _p.uniqueness_ratio);
  _p.speckle_window_size = cf.get<int>("speckleWindowSize", _p.speckle_window_size);
  _p.speckle_range = cf.get<int>("speckleRange", _p.speckle_range);
  _p.try_smaller_windows = cf.get<int>("trySmallerWindows", _p.try_smaller_windows);
  _p.disp12_max_diff = cf.get<int>("disp12MaxDiff", _p.disp12_max_diff);
  const int rc = pba_stereo_validate_params(0, 0, &_p);
  if (rc != PBA_OK) throw std::runtime_error("StereoAlgorithm: " + stereoError(rc, nullptr));
}

StereoAlgorithm::~StereoAlgorithm() { pba_stereo_destroy(_h); }

pba_stereo* StereoAlgorithm::handle(const ImageSize& size) {
  if (_h && size.rows == _size.rows && size.cols == _size.cols) return _h;
  pba_stereo_destroy(_h);
  _h = nullptr;
  const int rc = pba_stereo_create(size.rows, size.cols, &_p, _device, &_h);
  if (rc != PBA_OK) throw std::runtime_error("pba_stereo_create: " + stereoError(rc, nullptr));
  _size = size;
  return _h;
}

void StereoAlgorithm::run(const uint8_t* left, const uint8_t* right, const ImageSize& size, float* dmap) {
  pba_stereo* h = handle(size);
  std::vector<int16_t> d16((size_t)size.numel());
  const int rc = pba_stereo_compute(h, left, right, 1.0f, d16.data(), nullptr);
  if (rc != PBA_OK) throw std::runtime_error("pba_stereo_compute: " + stereoError(rc, h));
  for (size_t i = 0; i < d16.size(); ++i) dmap[i] = (float)d16[i] * 0.0625f;   // exact
}

void StereoAlgorithm::run(const Image_<uint8_t>& left, const Image_<uint8_t>& right, float* dmap) {
  if (left.rows() != right.rows() || left.cols() != right.cols()) throw std::runtime_error("StereoAlgorithm::run: image sizes differ");
  run(left.data(), right.data(), ImageSize(left.rows(), left.cols()), dmap);
}

void StereoAlgorithm::depth(const uint8_t* left, const uint8_t* right, const ImageSize& size, float Bf, float* zmap) {
  pba_stereo* h = handle(size);
  const int rc = pba_stereo_compute(h, left, right, Bf, nullptr, zmap);
  if (rc != PBA_OK) throw std::runtime_error("pba_stereo_compute: " + stereoError(rc, h));
}

float StereoAlgorithm::getInvalidValue() const { return (float)(_p.min_disparity - 1); }
