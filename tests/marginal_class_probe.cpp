// Stand-alone program around Options::marginalize of the host class (photobundle_amd/host/photobundle.h): the ConfigFile key and its
// default, the line operator<< prints, the Result field, and the three std::invalid_argument cases -- with camerasConstant, with
// computeCovariance (both thrown by the constructor before it touches a device) and from addFrames, which needs an instance and so a
// device: without one the program says "addFrames skipped" and the GPU suite runs it again.  One line per finding on standard output;
// the exit status is 0 when every check that could run passed.
#include <cstdio>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "../photobundle_amd/host/photobundle.h"
#include "../photobundle_amd/host/utils.h"

typedef PhotometricBundleAdjustment PBA;

static PBA::Options options(bool marginalize) {
  PBA::Options o;
  o.slidingWindowSize = 4; o.patchRadius = 1; o.verbose = false; o.marginalize = marginalize;
  return o;
}

// "invalid_argument" | "other: <what>" | "none"
static std::string construct(const PBA::Options& o, std::unique_ptr<PBA>* keep = nullptr) {
  Calibration calib;
  const double c5[5] = {160.0, 160.0, 64.0, 48.0, 0.5};
  calib.setParameters(c5);
  try {
    std::unique_ptr<PBA> ba(new PBA(calib, ImageSize(96, 128), o));
    if (keep) *keep = std::move(ba);
    return "none";
  } catch (const std::invalid_argument& ex) {
    return std::string("invalid_argument: ") + ex.what();
  } catch (const std::exception& ex) {
    return std::string("other: ") + ex.what();
  }
}

int main() {
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { std::printf("%s %s\n", ok ? "ok" : "FAILED", what); if (!ok) ++bad; };
  // the key and its default
  utils::ConfigFile cf;
  expect(!PBA::Options().marginalize && !PBA::Options(cf).marginalize, "default 0");
  cf("marginalize", "1");
  expect(PBA::Options(cf).marginalize, "key marginalize = 1");
  cf("Marginalize", "0");
  expect(!PBA::Options(cf).marginalize, "key marginalize = 0");
  std::ostringstream on, off;
  on << options(true);
  off << options(false);
  expect(on.str().find("\nmarginalize = 1\n") != std::string::npos && off.str().find("\nmarginalize = 0\n") != std::string::npos, "operator<< prints the key");
  expect(PBA::Result().priorCost == 0.0, "Result::priorCost defaults to 0");
  // the constructor's two refusals, before any device call
  PBA::Options o = options(true);
  o.camerasConstant = true;
  std::string r = construct(o);
  std::printf("with camerasConstant: %s\n", r.c_str());
  expect(r.rfind("invalid_argument: marginalize with camerasConstant", 0) == 0, "invalid_argument with camerasConstant");
  o = options(true);
  o.computeCovariance = true; o.numConstantFrames = 2;
  r = construct(o);
  std::printf("with computeCovariance: %s\n", r.c_str());
  expect(r.rfind("invalid_argument: marginalize with computeCovariance", 0) == 0, "invalid_argument with computeCovariance");
  // addFrames: an instance needs a device
  std::unique_ptr<PBA> ba;
  r = construct(options(true), &ba);
  if (!ba) {
    std::printf("addFrames skipped: %s\n", r.c_str());
    expect(r.rfind("other: ", 0) == 0 && r.find("pba_create") != std::string::npos, "marginalize alone passes the constructor's checks");
  } else {
    std::vector<uint8_t> img(96 * 128, 0);
    std::vector<float> depth(96 * 128, 1.0f);
    const Mat44 T = Mat44::Identity();
    std::string got = "none";
    try {
      PBA::addFrames({ba.get()}, {PBA::Frame{img.data(), depth.data(), &T}}, {});
    } catch (const std::invalid_argument& ex) {
      got = std::string("invalid_argument: ") + ex.what();
    } catch (const std::exception& ex) {
      got = std::string("other: ") + ex.what();
    }
    std::printf("addFrames: %s\n", got.c_str());
    expect(got.rfind("invalid_argument: addFrames: Options::marginalize solves alone", 0) == 0, "invalid_argument from addFrames");
  }
  return bad ? 1 : 0;
}
