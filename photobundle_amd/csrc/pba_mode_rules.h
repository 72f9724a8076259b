// pba_mode_rules.h -- THE table of features that do not combine, with the sentence each refusal says.  A row names two features and
// holds one sentence per call order: `then_b` is said when `a` is present and `b` is switched on, `then_a` the other way round.  A row
// without a second sentence has a `b` that is never present when something is switched on (the sampler flags are fixed at pba_create;
// the covariance output, a batch and a cull are calls, not states): asked the other way round it answers with the same sentence.  The caller
// adds its prefix ("pba_set_cameras_constant: ") and suffix ("(%d free cameras)") and decides what counts as present (multi-rank:
// comm.multi() in the setters, world > 1 at pba_comm_init_*).  With several conflicts present the first row wins: the order of the
// rows is part of the interface.  No HIP header is needed: plain C++ compiles it (tests/mode_rules_probe.cpp does).
#pragma once

namespace pba {

enum ModeFeature : unsigned {      // one bit each
  kModeMulti = 1, kModeInverseDepth = 2, kModeSweep = 4 /* pba_config.flags bits 1-2 */, kModeWide = 8, kModePointsConst = 16, kModeCamsConst = 32,
  kModeAnchors = 64 /* two or more constant slots */, kModeCovariance = 128 /* pba_covariance */, kModeBatch = 256 /* pba_solve_batch */,
  kModePrior = 512 /* pba_set_camera_prior; pba_marginalize asks as if it switched one on */, kModeCull = 1024 /* pba_cull */,
  kModeAdmit = 2048 /* pba_admit */, kModePointPrior = 4096 /* pba_set_point_prior */
};
struct ModeRule { unsigned a, b; const char* then_b; const char* then_a; };
constexpr ModeRule kModeRules[] = {
    {kModeMulti, kModeWide, "multi-rank solves (pba_comm_*) are not built for wide windows", "multi-rank solves are not built for wide windows"},
    {kModeInverseDepth, kModeWide, "the inverse-depth mode (pba_set_inverse_depth) is not built for wide windows", "the inverse-depth mode is not built for wide windows"},
    {kModeWide, kModeSweep, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for wide windows", nullptr},
    {kModeMulti, kModePointsConst, "multi-rank solves (pba_comm_*) are not built for the points-constant mode",
     "multi-rank solves are not built for the points-constant mode (pba_set_points_constant)"},
    {kModePointsConst, kModeSweep, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for the points-constant mode", nullptr},
    {kModePointsConst, kModeCamsConst, "the points-constant mode (pba_set_points_constant) is on: with every block constant the program is empty",
     "the cameras-constant mode (pba_set_cameras_constant) is on: with every block constant the program is empty"},
    {kModeMulti, kModeCamsConst, "multi-rank solves (pba_comm_*) are not built for the cameras-constant mode",
     "multi-rank solves are not built for the cameras-constant mode (pba_set_cameras_constant)"},
    {kModeCamsConst, kModeSweep, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for the cameras-constant mode", nullptr},
    {kModeMulti, kModeAnchors, "multi-rank solves (pba_comm_*) take at most one constant slot", "multi-rank solves take at most one constant slot"},
    {kModeAnchors, kModeSweep, "the precision-sweep sampler modes (pba_config.flags bits 1-2) take at most one constant slot", nullptr},
    {kModeMulti, kModeCovariance, "multi-rank engines (pba_comm_*) are not built for the covariance output", nullptr},
    {kModeSweep, kModeCovariance, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for the covariance output", nullptr},
    {kModeInverseDepth, kModeCovariance, "the inverse-depth mode (pba_set_inverse_depth) with free cameras is not built; the cameras-constant mode takes it", nullptr},
    {kModeMulti, kModeBatch, "multi-rank engines (pba_comm_*) solve alone", nullptr},
    {kModeWide, kModeBatch, "wide window", nullptr},
    {kModeSweep, kModeBatch, "the precision-sweep flags solve alone", nullptr},
    {kModePointsConst, kModeBatch, "the points-constant mode (pba_set_points_constant) solves alone", nullptr},
    {kModeCamsConst, kModeBatch, "the cameras-constant mode (pba_set_cameras_constant) solves alone", nullptr},
    {kModeMulti, kModePrior, "multi-rank solves (pba_comm_*) are not built for the camera prior", "multi-rank solves are not built for the camera prior (pba_set_camera_prior)"},
    {kModePrior, kModeSweep, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for the camera prior", nullptr},
    {kModePrior, kModeWide, "the camera prior (pba_set_camera_prior) is not built for wide windows", "the camera prior is not built for wide windows"},
    {kModePointsConst, kModePrior, "the camera prior is not built for the points-constant mode (pba_set_points_constant)",
     "the camera prior (pba_set_camera_prior) is not built for the points-constant mode"},
    {kModeCamsConst, kModePrior, "the camera prior is not built for the cameras-constant mode (pba_set_cameras_constant)",
     "the camera prior (pba_set_camera_prior) is not built for the cameras-constant mode"},
    {kModeInverseDepth, kModePrior, "the camera prior is not built for the inverse-depth mode (pba_set_inverse_depth)",
     "the camera prior (pba_set_camera_prior) is not built for the inverse-depth mode"},
    {kModePrior, kModeCovariance, "the camera prior (pba_set_camera_prior) is set: a covariance that ignored it would be wrong", nullptr},
    {kModePrior, kModeBatch, "the camera prior (pba_set_camera_prior) solves alone", nullptr},
    {kModeMulti, kModeCull, "multi-rank engines (pba_comm_*) are not built for culling: the order statistic would need an exchange", nullptr},
    {kModeSweep, kModeCull, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for culling", nullptr},
    // (the point prior's rows; no query matches one of them and a row of pba_admit at once, and tests/test_admit_cpu.py pins those two as the last)
    {kModeMulti, kModePointPrior, "multi-rank solves (pba_comm_*) are not built for the point prior", "multi-rank solves are not built for the point prior (pba_set_point_prior)"},
    {kModePointPrior, kModeSweep, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for the point prior", nullptr},
    {kModePointPrior, kModeBatch, "the point prior (pba_set_point_prior) solves alone", nullptr},
    {kModePointsConst, kModePointPrior, "the point prior is not built for the points-constant mode (pba_set_points_constant): the prior is then a constant",
     "the point prior (pba_set_point_prior) is not built for the points-constant mode: the prior is then a constant"},
    {kModeInverseDepth, kModePointPrior, "the point prior is not built for the inverse-depth mode (pba_set_inverse_depth)",
     "the point prior (pba_set_point_prior) is not built for the inverse-depth mode"},
    {kModePrior, kModePointPrior, "the point prior is not built next to the camera prior (pba_set_camera_prior): it eliminates through the wide chain, the camera prior is narrow-only",
     "the camera prior is not built next to the point prior (pba_set_point_prior): it is narrow-only, the point prior eliminates through the wide chain"},
    {kModeMulti, kModeAdmit, "multi-rank engines (pba_comm_*) are not built for re-observation: the order statistic would need an exchange", nullptr},
    {kModeSweep, kModeAdmit, "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for re-observation", nullptr},
};

// Why feature `on` (one bit) cannot be switched on next to the features `present` (nullptr: it can); *with: the feature in its way
inline const char* mode_conflict(unsigned present, unsigned on, unsigned* with = nullptr) {
  for (const ModeRule& r : kModeRules) {
    const bool fwd = r.b == on && (present & r.a), bwd = r.a == on && (present & r.b);
    if (!fwd && !bwd) continue;
    if (with) *with = fwd ? r.a : r.b;
    return (fwd || !r.then_a) ? r.then_b : r.then_a;
  }
  return nullptr;
}

}  // namespace pba
