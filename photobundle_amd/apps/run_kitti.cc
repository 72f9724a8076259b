// run_kitti.cc -- the reference's driver loop (reference apps/run_kitti.cc:17-59) on the MI355X engine.
//
// OpenCV is absent from this image, so frames come from a directory of PGM files instead of Dataset::Create:
//     <data>/image_%06d.pgm   binary PGM (P5, 8 bit), the left image
//     <data>/depth_%06d.bin   rows*cols float32 depth map (what disparityToDepth would hand over; <= 0 invalid)
//     <data>/right_%06d.pgm   the right image (DepthSource = stereo)
//     <data>/calib.txt        fx fy cx cy baseline, or KITTI's own "P0: <12 numbers>" / "P1: <12 numbers>" lines
//                             (K = P0[:, :3], baseline = -P1(0,3) / P1(0,0), reference src/dataset.cc:235-253)
// The config file is the reference's (config/kitti_stereo.cfg keys) plus `DataDirectory` and `DepthSource`; `Trajectory` is
// the KITTI pose text file of frame-to-frame initial poses (reference data/kitti_init_poor/*.txt).
//     DepthSource = files    (default) depth from depth_%06d.bin
//     DepthSource = stereo   depth from the left/right pair on the device: the config's StereoAlgorithm (BlockMatching, or
//                            SGM / SemiGlobalMatching with the reference's SgmStereo keys) + disparityToDepth with
//                            Bf = baseline * fx (reference apps/run_kitti.cc:29, src/dataset.cc:105-137)
//     InitialPose = trajectory  (default) every frame's initial pose comes from the `Trajectory` file; the sequence ends with it
//     InitialPose = track       the driver produces its own: from frame 2 on the start pose is the constant-velocity prediction from
//                            the two latest refined poses, refined by trackFrame (pose-only alignment against the scene points)
//                            before addFrame receives it.  `Trajectory` is optional and supplies frames 0 and 1 only (identity and
//                            zero motion without it); the sequence ends with the images.  Not available with -b.
#include <algorithm>
#include <array>
#include <cctype>
#include <csignal>
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../host/photobundle.h"
#include "../host/photobundle_pyramid.h"
#include "../host/pose_utils.h"
#include "../host/sgm_stereo.h"
#include "../host/stereo_algorithm.h"
#include "../host/utils.h"

static volatile bool gStop = false;
static void sigHandler(int) { gStop = true; }

static bool readPgm(const std::string& fn, std::vector<uint8_t>& img, int& rows, int& cols) {
  std::ifstream ifs(fn, std::ios::binary);
  if (!ifs.is_open()) return false;
  std::string magic;
  int maxval = 0;
  ifs >> magic;
  if (magic != "P5") return false;
  auto skip = [&]() { while (ifs.peek() == '#' || std::isspace(ifs.peek())) { if (ifs.peek() == '#') { std::string l; std::getline(ifs, l); } else ifs.get(); } };
  skip(); ifs >> cols; skip(); ifs >> rows; skip(); ifs >> maxval;
  ifs.get();
  if (maxval != 255) return false;
  img.resize((size_t)rows * cols);
  ifs.read(reinterpret_cast<char*>(img.data()), img.size());
  return (bool)ifs;
}

// "fx fy cx cy baseline", or the KITTI calib.txt layout when the first token is a "P0:"-style label
static Calibration loadCalibration(const std::string& fn) {
  std::ifstream ifs(fn);
  std::string first;
  if (!(ifs >> first)) throw std::runtime_error("bad calib.txt");
  Calibration calib;
  if (first.back() == ':') {
    double P[2][12];
    for (int k = 0; k < 12; ++k)
      if (!(ifs >> P[0][k])) throw std::runtime_error("bad calib.txt: " + first + " needs 12 numbers");
    std::string second;
    if (!(ifs >> second) || second.back() != ':') throw std::runtime_error("bad calib.txt: no second camera line");
    for (int k = 0; k < 12; ++k)
      if (!(ifs >> P[1][k])) throw std::runtime_error("bad calib.txt: " + second + " needs 12 numbers");
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) calib.K()(r, c) = P[0][r * 4 + c];
    calib.baseline() = -P[1][3] / P[1][0];
    return calib;
  }
  double c5[5];
  std::istringstream first_ss(first);
  if (!(first_ss >> c5[0]) || !(ifs >> c5[1] >> c5[2] >> c5[3] >> c5[4])) throw std::runtime_error("bad calib.txt");
  calib.setParameters(c5);
  calib.baseline() = c5[4];
  return calib;
}

// prior: the sequence runs with marginalize = 1 (one more line, the E of the prior the optimisation carried)
// culled: the sequence runs with outlierPasses > 0 (one more line, the residual blocks and points the optimisation's culls removed)
// admitted: the sequence runs with reobservePasses > 0 (one more line, the residual blocks the optimisation's admissions added)
// depth_prior: the sequence runs with depthPriorSigma > 0 (one more line, the depth factors' share of the final cost)
static void dumpResult(const std::string& fn, int frame, const PhotometricBundleAdjustment::Result& r, bool prior = false, bool culled = false,
                       bool admitted = false, bool depth_prior = false) {
  std::FILE* f = std::fopen(fn.c_str(), "a");
  if (!f) throw std::runtime_error("cannot open " + fn);
  std::fprintf(f, "result frame %d poses %zu points %zu iterations %zu\n", frame, r.poses.size(), r.refinedPoints.size(), r.iterationSummary.size());
  std::fprintf(f, "cost %.17g %.17g %.17g steps %d residuals %d\n", r.initialCost, r.finalCost, r.fixedCost, r.numSuccessfulStep, r.numResiduals);
  if (prior) std::fprintf(f, "prior %.17g\n", r.priorCost);
  if (culled) std::fprintf(f, "culled blocks %d points %d\n", r.numCulledBlocks, r.numCulledPoints);
  if (admitted) std::fprintf(f, "admitted blocks %d\n", r.numAdmittedBlocks);
  if (depth_prior) std::fprintf(f, "depthPrior %.17g\n", r.depthPriorCost);
  std::fprintf(f, "message %s\n", r.message.c_str());
  for (const auto& it : r.iterationSummary)
    std::fprintf(f, "it %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", it.iteration, (int)it.step_is_valid, (int)it.step_is_successful, it.cost,
                 it.cost_change, it.gradient_max_norm, it.step_norm, it.relative_decrease, it.trust_region_radius);
  // every pose of the trajectory so far, round-trip precision (photobundle.cc:858: Result::poses covers all frames)
  for (size_t i = 0; i < r.poses.size(); ++i) {
    std::fprintf(f, "pose %zu", i);
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 4; ++b) std::fprintf(f, " %.17g", r.poses[i](a, b));
    std::fprintf(f, "\n");
  }
  for (size_t i = 0; i < r.refinedPoints.size(); ++i)
    std::fprintf(f, "pt %.17g %.17g %.17g %.17g %.17g %.17g\n", r.refinedPoints[i][0], r.refinedPoints[i][1], r.refinedPoints[i][2],
                 r.originalPoints[i][0], r.originalPoints[i][1], r.originalPoints[i][2]);
  std::fclose(f);
}

// One sequence: its config, data, initial trajectory and depth source (what main() reads for the single run, and per -b entry)
struct Sequence {
  std::unique_ptr<utils::ConfigFile> cf;
  std::string data, depth_source, output, results, initial_pose;
  bool track = false;
  Calibration calib;
  EigenAlignedContainer_<Mat44> T_init;
  std::vector<uint8_t> img, right;
  std::vector<float> depth;
  int rows = 0, cols = 0, num_levels = 1;
  float Bf = 0.f;
  std::unique_ptr<StereoAlgorithm> stereo;
  std::unique_ptr<SgmStereo> sgm;

  explicit Sequence(const std::string& config) : cf(new utils::ConfigFile(config)) {
    initial_pose = cf->get<std::string>("InitialPose", "trajectory");
    std::transform(initial_pose.begin(), initial_pose.end(), initial_pose.begin(), [](unsigned char c) { return std::tolower(c); });
    if (initial_pose != "trajectory" && initial_pose != "track") throw std::runtime_error("InitialPose must be trajectory or track, not " + initial_pose);
    track = initial_pose == "track";
    data = cf->get<std::string>("DataDirectory");
    calib = loadCalibration(data + "/calib.txt");
    depth_source = cf->get<std::string>("DepthSource", "files");
    std::transform(depth_source.begin(), depth_source.end(), depth_source.begin(), [](unsigned char c) { return std::tolower(c); });
    if (depth_source != "files" && depth_source != "stereo") throw std::runtime_error("DepthSource must be files or stereo, not " + depth_source);
    if (!track) T_init = loadPosesKittiFormat(cf->get<std::string>("trajectory"));
    else if (!cf->get<std::string>("trajectory", "").empty()) T_init = loadPosesKittiFormat(cf->get<std::string>("trajectory"));
    char name[64];
    std::snprintf(name, sizeof(name), "/image_%06d.pgm", 0);
    if (!readPgm(data + name, img, rows, cols)) throw std::runtime_error("cannot read the first frame");
    Bf = (float)(calib.b() * calib.fx());
    num_levels = cf->get<int>("numLevels", 1);   // > 1: coarse-to-fine (photobundle_pyramid path)
  }
  // StereoAlgorithm = SGM | SemiGlobalMatching builds the semi-global matcher; every other value goes to StereoAlgorithm
  void start() {
    if (depth_source != "stereo") return;
    if (SgmStereo::selectedBy(*cf)) sgm.reset(new SgmStereo(SgmStereo::Config::fromConfigFile(*cf)));
    else stereo.reset(new StereoAlgorithm(*cf));
  }
  // frame f_i into img / depth; false when the image is missing (the sequence ends)
  bool read(int f_i) {
    char name[64];
    std::snprintf(name, sizeof(name), "/image_%06d.pgm", f_i);
    int r2, c2;
    if (!readPgm(data + name, img, r2, c2)) return false;
    if (r2 != rows || c2 != cols) throw std::runtime_error("frame size changed");
    depth.resize((size_t)rows * cols);
    if (stereo || sgm) {
      std::snprintf(name, sizeof(name), "/right_%06d.pgm", f_i);
      if (!readPgm(data + name, right, r2, c2)) throw std::runtime_error(std::string("cannot read ") + (name + 1));
      if (r2 != rows || c2 != cols) throw std::runtime_error("right frame size differs");
      if (sgm) sgm->depth(img.data(), right.data(), ImageSize(rows, cols), Bf, depth.data());
      else stereo->depth(img.data(), right.data(), ImageSize(rows, cols), Bf, depth.data());
    } else {
      std::snprintf(name, sizeof(name), "/depth_%06d.bin", f_i);
      std::ifstream dfs(data + name, std::ios::binary);
      if (!dfs.read(reinterpret_cast<char*>(depth.data()), depth.size() * sizeof(float))) throw std::runtime_error("bad depth file");
    }
    return true;
  }
};

static void writePoses(const std::string& output, const PhotometricBundleAdjustment::Result& result, bool full_precision) {
  std::fprintf(stderr, "Writing refined poses to %s\n", output.c_str());
  if (full_precision) writePosesKittiFormatFullPrecision(output, result.poses);
  else writePosesKittiFormat(output, result.poses);   // reference format (src/pose_utils.cc:43-59)
}

// -b: several sequences from one process.  They advance in lockstep, one frame each, then one batched optimisation
// (PhotometricBundleAdjustment::addFrames); a sequence leaves when its frames or its trajectory run out.
static int runBatch(std::vector<std::unique_ptr<Sequence>>& seqs, bool full_precision) {
  for (auto& q : seqs)
    if (q->num_levels > 1) { std::fprintf(stderr, "error: -b takes single-level configs only (%s: numLevels = %d)\n", q->output.c_str(), q->num_levels); return 1; }
  std::vector<std::unique_ptr<PhotometricBundleAdjustment>> pb;
  std::vector<PhotometricBundleAdjustment::Result> res(seqs.size());
  std::vector<bool> live(seqs.size(), true);
  for (auto& q : seqs) { q->start(); pb.emplace_back(new PhotometricBundleAdjustment(q->calib, ImageSize(q->rows, q->cols), {*q->cf})); }
  for (int f_i = 0; !gStop; ++f_i) {
    std::vector<PhotometricBundleAdjustment*> inst;
    std::vector<PhotometricBundleAdjustment::Frame> frames;
    std::vector<PhotometricBundleAdjustment::Result*> out;
    std::vector<size_t> idx;
    for (size_t k = 0; k < seqs.size(); ++k) {
      if (!live[k]) continue;
      if (f_i >= (int)seqs[k]->T_init.size() || !seqs[k]->read(f_i)) { live[k] = false; writePoses(seqs[k]->output, res[k], full_precision); continue; }
      res[k].initialCost = -1.0;
      inst.push_back(pb[k].get());
      frames.push_back({seqs[k]->img.data(), seqs[k]->depth.data(), &seqs[k]->T_init[f_i]});
      out.push_back(&res[k]);
      idx.push_back(k);
    }
    if (inst.empty()) break;
    std::printf("Frame %05d (%zu sequences)\n", f_i, inst.size());
    PhotometricBundleAdjustment::addFrames(inst, frames, out);
    for (size_t k : idx)
      if (!seqs[k]->results.empty() && res[k].initialCost >= 0.0) dumpResult(seqs[k]->results, f_i, res[k]);
  }
  for (size_t k = 0; k < seqs.size(); ++k) if (live[k]) writePoses(seqs[k]->output, res[k], full_precision);
  return 0;
}

int main(int argc, char** argv) {
  signal(SIGINT, sigHandler);
  // -r (not in the reference's driver): text dump of every Result the class hands back (reference photobundle.cc:857-875)
  // -p (not in the reference's driver): poses with round-trip precision instead of the reference's 6 significant digits
  // -b CONFIG:OUTPUT[:RESULTS] (not in the reference's driver, repeatable): several sequences from one process (runBatch)
  std::string config = "../config/kitti_stereo.cfg", output = "refined_poses.txt", results;
  bool full_precision = false, single_opts = false;
  std::vector<std::string> batch;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if ((a == "-c" || a == "--config") && i + 1 < argc) { config = argv[++i]; single_opts = true; }
    else if ((a == "-o" || a == "--output") && i + 1 < argc) { output = argv[++i]; single_opts = true; }
    else if ((a == "-r" || a == "--results") && i + 1 < argc) { results = argv[++i]; single_opts = true; }
    else if (a == "-p" || a == "--full-precision") full_precision = true;
    else if ((a == "-b" || a == "--batch") && i + 1 < argc) batch.push_back(argv[++i]);
    else { std::fprintf(stderr, "usage: %s [-c config] [-o output] [-r result-dump] [-p]  |  %s -b config:output[:result-dump] [-b ...] [-p]\n", argv[0], argv[0]); return 1; }
  }
  if (!batch.empty()) {
    if (single_opts) { std::fprintf(stderr, "error: -b names each sequence's config, output and result dump; it does not combine with -c, -o or -r\n"); return 1; }
    std::vector<std::array<std::string, 3>> specs;
    for (const std::string& b : batch) {
      std::array<std::string, 3> f;
      size_t n_f = 0, pos = 0;
      while (n_f < 3) {
        const size_t c = b.find(':', pos);
        f[n_f++] = b.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
        if (c == std::string::npos) break;
        pos = c + 1;
        if (n_f == 3) { n_f = 4; break; }
      }
      if (n_f < 2 || n_f > 3 || f[0].empty() || f[1].empty() || (n_f == 3 && f[2].empty())) {
        std::fprintf(stderr, "error: -b takes CONFIG:OUTPUT[:RESULTS], got \"%s\"\n", b.c_str());
        return 1;
      }
      specs.push_back(f);
    }
    try {
      std::vector<std::unique_ptr<Sequence>> seqs;
      for (const auto& f : specs) {
        seqs.emplace_back(new Sequence(f[0]));
        seqs.back()->output = f[1];
        seqs.back()->results = f[2];
        if (seqs.back()->track) { std::fprintf(stderr, "error: -b does not take InitialPose = track (%s): the batched driver has no tracker\n", f[0].c_str()); return 1; }
      }
      return runBatch(seqs, full_precision);
    } catch (const std::exception& ex) {
      std::fprintf(stderr, "error: %s\n", ex.what());
      return 1;
    }
  }
  try {
    Sequence q(config);
    q.start();
    const int rows = q.rows, cols = q.cols;
    PhotometricBundleAdjustment::Result result;
    std::unique_ptr<PhotometricBundleAdjustment> photoba;
    std::unique_ptr<PhotometricBundleAdjustmentPyr> photoba_pyr;
    if (q.num_levels > 1) photoba_pyr.reset(new PhotometricBundleAdjustmentPyr(q.num_levels, q.calib, ImageSize(rows, cols), {*q.cf}));
    else photoba.reset(new PhotometricBundleAdjustment(q.calib, ImageSize(rows, cols), {*q.cf}));
    const bool with_prior = PhotometricBundleAdjustment::Options(*q.cf).marginalize;
    // outlierPasses > 0: optimize() culls after its solve, and so does the tracker of InitialPose = track (TrackOptions::outlierPasses)
    const int outlier_passes = PhotometricBundleAdjustment::Options(*q.cf).outlierPasses;
    TrackOptions track_options;
    track_options.outlierPasses = outlier_passes;
    const int reobserve_passes = PhotometricBundleAdjustment::Options(*q.cf).reobservePasses;
    const bool depth_prior = PhotometricBundleAdjustment::Options(*q.cf).depthPriorSigma > 0.0;
    Mat44 T_last = Mat44::Identity();      // (InitialPose = track) the frame-to-frame pose the previous frame was added with
    for (int f_i = 0; (q.track || f_i < (int)q.T_init.size()) && !gStop; ++f_i) {
      if (!q.read(f_i)) break;
      std::printf("Frame %05d\n", f_i);
      Mat44 T = f_i < (int)q.T_init.size() ? q.T_init[f_i] : Mat44::Identity();
      if (q.track && f_i >= 2) {
        // constant velocity: the latest refined frame-to-frame motion repeats (T_i = inv(T_w_i) * T_w_(i-1), trajectory.h); before the
        // first optimisation no pose has been refined and the motion the previous frame was added with stands in
        const size_t m = result.poses.size();
        const Mat44 T_pred = m >= 2 ? Mat44(result.poses[m - 1].inverse() * result.poses[m - 2]) : T_last;
        TrackResult tr;
        T = photoba_pyr ? photoba_pyr->trackFrame(q.img.data(), T_pred, track_options, &tr) : photoba->trackFrame(q.img.data(), T_pred, track_options, &tr);
        if (!tr.tracked) {
          std::fprintf(stderr, "frame %d was not tracked (%s): keeping the constant-velocity prediction\n", f_i, tr.message.c_str());
          T = T_pred;
        }
        std::printf("track frame %d tracked %d points %d iterations %d cost %.6e -> %.6e pose", f_i, (int)tr.tracked, tr.numPoints, tr.numIterations,
                    tr.initialCost, tr.finalCost);
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 4; ++b) std::printf(" %.17g", T(a, b));
        std::printf("\n");
        if (outlier_passes > 0) std::printf("track frame %d culled blocks %d points %d\n", f_i, tr.numCulledBlocks, tr.numCulledPoints);
      }
      T_last = T;
      result.initialCost = -1.0;    // the class only touches `result` when an optimisation ran (photobundle.cc:857)
      if (photoba_pyr) photoba_pyr->addFrame(q.img.data(), q.depth.data(), T, &result);
      else photoba->addFrame(q.img.data(), q.depth.data(), T, &result);
      if (!results.empty() && result.initialCost >= 0.0) dumpResult(results, f_i, result, with_prior, outlier_passes > 0, reobserve_passes > 0, depth_prior);
    }
    writePoses(output, result, full_precision);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  return 0;
}
