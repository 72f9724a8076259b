// photobundle.h -- the reference's public class, MI355X engine underneath.
//
// Same class name, nested types, field names, defaults and call signatures as reference src/photobundle.h:19-196, so
// that apps/run_kitti.cc-style callers compile against it unchanged:
//
//     PhotometricBundleAdjustment photoba(calib, image_size, {cf});
//     photoba.addFrame(I, Z, T_init[f_i], &result);
//
// What changed underneath: the Ceres problem / ceres::Solve block of optimize() (reference src/photobundle.cc:784-829)
// is replaced by the C-ABI engine of include/pba.h (hand-written HIP for gfx950); Eigen / boost / ceres types in the
// header are replaced by the stand-ins of types.h and the ceres::IterationSummary struct below.
#ifndef PHOTOBUNDLE_AMD_PHOTOBUNDLE_H
#define PHOTOBUNDLE_AMD_PHOTOBUNDLE_H

#include <cstdint>
#include <iosfwd>
#include <string>
#include <utility>
#include <vector>

#include "calibration.h"
#include "trajectory.h"
#include "types.h"

namespace utils { class ConfigFile; }

namespace ceres {
// The fields the reference reads / serialises (reference src/ceres_cereal.h:13-30), same names.
struct IterationSummary {
  int iteration = 0;
  bool step_is_valid = false;
  bool step_is_nonmonotonic = false;
  bool step_is_successful = false;
  double cost = 0.0;
  double cost_change = 0.0;
  double gradient_max_norm = 0.0;
  double gradient_norm = 0.0;
  double step_norm = 0.0;
  double relative_decrease = 0.0;
  double trust_region_radius = 0.0;
  double eta = 0.0;
  double step_size = 0.0;
  int line_search_function_evaluations = 0;
  int line_search_gradient_evaluations = 0;
  int line_search_iterations = 0;
  int linear_solver_iterations = 0;
  double iteration_time_in_seconds = 0.0;
  double step_solver_time_in_seconds = 0.0;
  double cumulative_time_in_seconds = 0.0;
};
}  // namespace ceres

struct pba_engine;
class PhotometricBundleAdjustmentPyr;

// ---- trackFrame (new; not in the reference): align one frame to the scene points, which stay put ----
struct TrackOptions {
  int maxIterations = 50;
  int minPoints = 64;                 // below it the frame is not tracked
  bool computeCovariance = false;     // pba_covariance after the alignment: the 6x6 covariance of the tracked pose
  // outlier culling (new): after the alignment up to outlierPasses rounds of pba_cull + pba_solve, pose-only (every point has one block
  // here, so a point stays with one surviving block: min_observations = 1); threshold from Options::outlierQuantile / outlierFactor /
  // outlierMinCost of the instance.  Stops early when a cull removes nothing (or would remove everything).  0: as without the field.
  int outlierPasses = 0;
};
struct TrackResult {
  bool tracked = false;
  int numPoints = 0;                  // scene points inside the border under T_init (one residual block each)
  double initialCost = -1.0, finalCost = -1.0;
  int numIterations = 0;
  std::string message;
  int numCulledBlocks = 0, numCulledPoints = 0;   // TrackOptions::outlierPasses: summed over the passes (costs, iterations and message: the last solve's;
                                                  // initialCost: the first solve's)
  // TrackOptions::computeCovariance: (J^T J)^-1 of the tracked camera, row-major 6x6, unit residual variance, in the engine's camera
  // parameters (angle-axis and translation of the WORLD->CAMERA transform, not the frame-to-frame pose trackFrame returns); minPivot is
  // the smallest Cholesky pivot of its unit-diagonal form, in (0, 1].  covarianceOk = false: not asked for, not tracked, or the call
  // failed -- covarianceMessage then holds the engine's status and message (singular against refused).
  bool covarianceOk = false;
  std::string covarianceMessage;
  double covariance[36] = {0};
  double minPivot = 0.0;
};

// Same public surface as the reference class (nested Options / Result, addFrame, protected optimize); the private
// part is this implementation's own.
class PhotometricBundleAdjustment {
 public:
  struct Options;
  struct Result;

  PhotometricBundleAdjustment(const Calibration& calibration, const ImageSize& image_size, const Options& options);
  PhotometricBundleAdjustment(const Calibration& calibration, const ImageSize& image_size);
  ~PhotometricBundleAdjustment();
  PhotometricBundleAdjustment(const PhotometricBundleAdjustment&) = delete;
  PhotometricBundleAdjustment& operator=(const PhotometricBundleAdjustment&) = delete;

  // image: dense row-major rows x cols u8; depth_map: dense row-major float (<= 0 / out of [minValidDepth,
  // maxValidDepth] = invalid); T: frame-to-frame pose initialisation.  `result` (optional) is overwritten whenever
  // an optimisation ran, i.e. once the sliding window is full.
  void addFrame(const uint8_t* image, const float* depth_map, const Mat44& T, Result* result = nullptr);

  // Pose-only alignment (new): refines the frame-to-frame pose `T_init` of `image` -- the argument addFrame would take for this
  // frame, and the return value is in the same convention -- against the scene points the instance holds now, every point
  // constant (pba_set_points_constant).  Every scene point whose projection under T_init lies inside the border of addFrame's
  // visibility test carries its stored descriptor as one residual block.  Touches neither the window, the trajectory, the mask,
  // the scene points nor the bundle-adjustment engine: it runs on a two-slot engine of its own, created at the first call.  With
  // fewer than minPoints points it returns T_init and tracked = false.
  Mat44 trackFrame(const uint8_t* image, const Mat44& T_init, const TrackOptions& options = TrackOptions(), TrackResult* result = nullptr);

  // Diagnostics (new): the visibility list of every scene point the instance holds, in the order it holds them -- the ids of the frames
  // whose residual blocks the point has, ascending.
  std::vector<std::vector<uint32_t>> visibilityLists() const;

  // Several independent sequences in lockstep (new): addFrame's front-end for every instance, then ONE pba_solve_batch per kernel key
  // (patch radius, descriptor channels, Gaussian weighting) over every instance whose window is full, then each instance's read-back,
  // eviction and Result.  Each instance ends exactly where its own addFrame would.  frames[i] / results[i] (results may be empty or hold
  // nulls) belong to instances[i]; instances appear once each.  A group the batch refuses is solved instance by instance.
  struct Frame { const uint8_t* image; const float* depth_map; const Mat44* T; };
  static void addFrames(const std::vector<PhotometricBundleAdjustment*>& instances, const std::vector<Frame>& frames,
                        const std::vector<Result*>& results);

  // ---- solver / front-end settings: field names, meanings and ConfigFile keys of the reference ----
  struct Options {
    // front-end
    int maxNumPoints = 4096;          // new scene points kept per frame (largest saliency first)
    int nonMaxSuppRadius = 1;         // saliency non-maximum suppression radius
    int maskBlockRadius = 1;          // pixels blocked around a re-observed point
    int maxFrameDistance = 1;         // a point not seen for more frames than this is no longer tracked
    double minScore = 0.75;           // ZNCC acceptance threshold, in [-1, 1]
    double minValidDepth = 0.01;
    double maxValidDepth = 1000.0;
    // problem shape
    int slidingWindowSize = 5;
    int patchRadius = 2;
    bool doGaussianWeighting = false;
    double robustThreshold = 0.05;    // Huber threshold; <= 0 disables the loss
    enum class DescriptorType { Intensity, IntensityAndGradient, BitPlanes };
    DescriptorType descriptorType = DescriptorType::Intensity;   // (left uninitialised by the reference)
    // execution
    int numThreads = -1;              // accepted for source compatibility; the solve runs on the GPU
    bool verbose = true;
    int device = 0;                   // HIP device ordinal (new)
    // structure-only refinement (new): every camera is a constant parameter block (pba_set_cameras_constant), the optimisation
    // refines the scene points against the trajectory exactly as the inputs chained it
    bool camerasConstant = false;
    // anchor frames (new): optimize() holds the min(numConstantFrames, frames in the window - 1) OLDEST frames of the window constant
    // (pba_set_cameras_anchored).  1 is the reference's behaviour (:809-813); valid values are 1 .. slidingWindowSize - 1, anything
    // else throws std::invalid_argument when the class is constructed.  trackFrame is not affected.
    int numConstantFrames = 1;
    // covariance output (new): pba_covariance after every optimisation, into Result.  Needs a fixed gauge: numConstantFrames >= 2,
    // camerasConstant, or depthPriorSigma > 0 (the depth factors fix the scale); with one constant frame and none of these the scale of
    // the window is free and the normal matrix singular, so the constructor throws std::invalid_argument.  Off: the class produces
    // what it produced without the field.
    bool computeCovariance = false;
    // marginalisation prior (new): before optimize() evicts the oldest frame's points it keeps what they said about the remaining
    // cameras as a quadratic prior (pba_marginalize on the oldest frame's ring slot), and the next window's optimisation carries it as
    // one more residual block on those cameras (pba_set_camera_prior).  Priors chain from window to window.  Throws
    // std::invalid_argument together with camerasConstant or computeCovariance (the constructor) and from addFrames (the batch).  A
    // marginalisation that fails (a singular block) clears the prior, says so on stderr and does not stop the run.  Off: the class
    // produces what it produced without the field.
    bool marginalize = false;
    // outlier culling (new; the step the reference leaves as a TODO after its solve): after pba_solve, optimize() runs pba_cull then
    // pba_solve again, up to outlierPasses times, and stops early when a cull removes nothing.  A residual block goes when its
    // loss-corrected cost exceeds max(outlierMinCost, outlierFactor x the outlierQuantile-quantile of all block costs); a point that keeps
    // fewer than outlierMinObservations blocks goes with all of them (include/pba.h, pba_cull).  The frame of every removed block leaves
    // the scene point's visibility list, so later windows do not add it again; the point's REFERENCE frame stays in the list (it decides
    // when the point is evicted) and is only marked, which keeps its block out as well.  Covariance and marginalisation see the culled
    // problem.  The last four are read only when outlierPasses > 0; their defaults are untuned on real imagery.  Ranges (else
    // std::invalid_argument from the constructor): outlierPasses >= 0, outlierQuantile in [0, 1], outlierFactor >= 0 and finite,
    // outlierMinCost >= 0 and finite, outlierMinObservations >= 1.  addFrames throws with outlierPasses > 0 (batched culling is not
    // built).  0: the class produces what it produced without the fields, and no new call reaches the engine.
    int outlierPasses = 0;
    double outlierQuantile = 0.5;
    double outlierFactor = 3.0;
    double outlierMinCost = 0.0;
    int outlierMinObservations = 2;
    // re-observation (new): a residual block enters through addFrame's one ZNCC test under the INITIAL pose; after pba_solve, and before
    // the outlier passes (so that a cull judges the admitted blocks too), optimize() runs pba_admit then pba_solve again, up to
    // reobservePasses times, and stops when a pass admits nothing.  Candidates are the (point, frame) pairs of the window that are not
    // residual blocks and whose projection at the refined state lies inside addFrame's border with depth >= minValidDepth; one is taken
    // when its loss-corrected cost is at most max(reobserveMinCost, reobserveFactor x the reobserveQuantile-quantile of the costs of the
    // blocks the problem already has) (include/pba.h, pba_admit).  Every admitted block adds its frame to its scene point's visibility
    // list, kept in ascending frame order: a point re-observed in the newest frame stays trackable under maxFrameDistance.  The last
    // three are read only when reobservePasses > 0; their defaults are untuned on real imagery.  Ranges (else std::invalid_argument from
    // the constructor): reobservePasses >= 0, reobserveQuantile in [0, 1], reobserveFactor >= 0 and finite, reobserveMinCost >= 0 and
    // finite.  addFrames throws with reobservePasses > 0.  0: the class produces what it produced without the fields, and no new call
    // reaches the engine.
    int reobservePasses = 0;
    double reobserveFactor = 1.0;
    double reobserveQuantile = 0.5;
    double reobserveMinCost = 0.0;
    // depth prior (new): every scene point keeps the stereo depth z0 it was created from as a factor (pba_set_point_prior).  The value is
    // the standard deviation of the DISPARITY in pixels; 0 switches the prior off.  Before the solve of every window, for every point of
    // the problem, with (R, t) the world->camera transform of the point's reference frame as this window starts from it:
    //   n = R^T e_z,  X0 = R^T (((x0 - cx) z0 / fx, (y0 - cy) z0 / fy, z0) - t),  sigma_z = depthPriorSigma z0^2 / (b fx),  Lambda = n n^T / sigma_z^2.
    // The reference frame is always part of the window, so the factor is re-expressed at that frame's latest pose every window: an
    // approximation of a camera-point depth factor, which would move with the camera inside the solve.  The engine carries the rows
    // through the outlier and re-observation passes.  std::invalid_argument from the constructor when the value is negative or not
    // finite, when it is positive and Calibration::b() <= 0, and together with marginalize (the engine refuses a camera prior next to
    // the point prior); from addFrames when it is positive (pba_solve_batch refuses it).  0: the class produces what it produced
    // without the field, and no new call reaches the engine.
    double depthPriorSigma = 0.0;

    Options() {}
    Options(const utils::ConfigFile& cf);

   private:
    // declared by the reference (src/photobundle.h:81-82) and never defined there: prints the settings as ConfigFile lines
    // (key = value, the keys Options(const ConfigFile&) reads), so that the output of one run configures the next
    friend std::ostream& operator<<(std::ostream&, const Options&);
  };

  // ---- what an optimisation reports ----
  struct Result {
    EigenAlignedContainer_<Mat44> poses;           // refined world poses of the whole trajectory so far
    EigenAlignedContainer_<Vec3> refinedPoints;    // points that left the window in this call ...
    EigenAlignedContainer_<Vec3> originalPoints;   // ... and what they were initialised to
    double initialCost = -1.0;
    double finalCost = -1.0;
    double fixedCost = -1.0;
    double priorCost = 0.0;                         // Options::marginalize: E of the prior this optimisation carried, at its final state
                                                    // (part of finalCost); 0 without a prior
    double depthPriorCost = 0.0;                    // Options::depthPriorSigma: the depth factors' share of finalCost, at the final state; 0 when off
    int numSuccessfulStep = 0;
    int numResiduals = 0;
    // Options::outlierPasses: residual blocks and points the culls of this optimisation removed, summed over the passes.  initialCost is
    // then the FIRST solve's; finalCost, numSuccessfulStep, numResiduals, totalTime, message and iterationSummary are the LAST solve's
    int numCulledBlocks = 0, numCulledPoints = 0;
    // Options::reobservePasses: residual blocks the admissions of this optimisation added, summed over the passes (the costs and the
    // other fields follow the rule above: initialCost the FIRST solve's, the rest the LAST solve's)
    int numAdmittedBlocks = 0;
    // ... and which: (position of the scene point in visibilityLists() as it stands after this call, frame id) of every admitted block
    // whose point is still held (the oldest frame's points have left by then), in the order of the admissions
    std::vector<std::pair<uint32_t, uint32_t>> admittedBlocks;
    double totalTime = -1.0;                       // seconds
    std::string message;
    std::vector<ceres::IterationSummary> iterationSummary;
    // Options::computeCovariance: blocks of (J^T J)^-1 at the refined state, unit residual variance (scale by your own sigma^2).
    // covarianceOk = false (with covarianceMessage) when the normal matrix was singular or the engine refused; the optimisation result
    // above is not affected.  minCameraPivot / minPointPivot: smallest Cholesky pivots of the unit-diagonal blocks, in (0, 1] -- a value
    // near rounding (1e-9 and below) means an inverse without meaning, the judgement is the caller's.
    // poseCovariance: n x n row-major, n = 6 x covarianceFrameIds.size(), the free frames of the window in ascending frame id (empty with
    // camerasConstant).  The parameters are the ENGINE's: angle-axis (3) and translation (3) of the WORLD->CAMERA transform of each
    // frame, NOT the coordinates of `poses` (camera->world matrices); the conversion is the caller's.
    // refinedPointCovariances: one 3x3 per entry of refinedPoints, same order (world coordinates); a point that was not part of the
    // optimisation has an all-zero block.
    bool covarianceOk = false;
    std::string covarianceMessage;
    double minCameraPivot = 0.0, minPointPivot = 0.0;
    std::vector<uint32_t> covarianceFrameIds;
    std::vector<double> poseCovariance;
    EigenAlignedContainer_<Mat33> refinedPointCovariances;

    // cereal-based serialisation is dead code in the reference's default build; kept as stubs for the signatures
    struct Writer {
      explicit Writer(std::string prefix = "./") : _counter(0), _prefix(prefix) {}
      bool add(const Result&);
     private:
      int _counter;
      std::string _prefix;
    };
    static Result FromFile(std::string);
  };

 protected:
  void optimize(Result*);

 private:
  struct ScenePoint;
  struct DescriptorFrame;
  struct OptimizeState;
  // addFrame in parts (addFrames runs them over several instances): the front-end returns whether an optimisation is due and, with
  // `defer`, leaves it to the caller; optimize = assemble (problem + cameras into the engine; false: nothing to solve), solve, finish
  bool addFrameImpl(const uint8_t* image, const float* depth_map, const Mat44& T, Result* result, bool defer);
  bool optimizeAssemble(OptimizeState& st);
  void optimizeFinish(OptimizeState& st, Result* result);
  void cullAndResolve(OptimizeState& st);      // Options::outlierPasses, between the solve and optimizeFinish
  void admitAndResolve(OptimizeState& st);     // Options::reobservePasses, between the solve and cullAndResolve
  // Options::depthPriorSigma: the depth factors of `selected` expressed at the cameras `cams` (what pba_set_point_prior takes)
  void depthPrior(const std::vector<ScenePoint*>& selected, const std::vector<double>& cams, std::vector<double>& x0, std::vector<double>& L6) const;
  typedef UniquePointer<ScenePoint> ScenePointPointer;
  typedef std::vector<ScenePointPointer> ScenePointPointerList;

  ScenePointPointerList removePointsAtFrame(uint32_t id);
  const DescriptorFrame* getFrameAtId(uint32_t id) const;

  uint32_t _frame_id = 0;
  Calibration _calib;
  ImageSize _image_size;
  UniquePointer<Options> _options_ptr;
  Trajectory _trajectory;
  std::vector<UniquePointer<DescriptorFrame>> _frame_buffer;   // the last slidingWindowSize frames, oldest first
  ScenePointPointerList _scene_points;
  Image_<uint16_t> _mask;
  Image_<float> _saliency_map;
  Mat33 _K_inv;
  pba_engine* _engine = nullptr;
  pba_engine* _track_engine = nullptr;                          // trackFrame's own (2 slots), created at its first call
  // set by the pyramid class when it has already put the next frame into the engine's ring slot on the device
  // (pba_set_frame_pyr_down): addFrame() then skips its own upload
  bool _frame_resident = false;
  // Options::marginalize: the prior the last optimisation left behind (pba_marginalize), set after the next window's cameras
  bool _prior_valid = false;
  std::vector<int32_t> _prior_slots;
  std::vector<double> _prior_x0, _prior_Lambda, _prior_eta;
  double _prior_c = 0.0;
  friend class PhotometricBundleAdjustmentPyr;
};

#endif
