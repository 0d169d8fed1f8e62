// The robust-round schedule of ObjectSLAM.optimize (lib/object_slam.py:842-896) and g2o's Levenberg-Marquardt damping schedule
// (optimization_algorithm_levenberg.cpp:58-175), written ONCE: the arithmetic as pure __host__ __device__ steps (no memory, no lanes), and the control
// flow of a whole run as one device template the one-launch kernels instantiate (csrc/lm_cam.hip, lm_cam2.hip, lm_frame.hip, lm_frame2.hip).
// csrc/lm.hip (its own loop, see there), the device state machine (csrc/lm_dist.hip: ba_ctl_lin, ba_decide) and the host loop (csrc/ba_drive.hip) call the steps; suo_slam_amd/ba_dist.py
// mirrors them in Python (bench.py holds it bit for bit against the C driver).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace suo {

#define LM_HD __host__ __device__ __forceinline__

constexpr int LM_MAX_TRIALS = 10;                       // g2o: _maxTrialsAfterFailure
constexpr int diag21[6] = {0, 6, 11, 15, 18, 20};       // the diagonal of a 6x6 block stored packed upper (21)

// ---- rounds ----
LM_HD int lm_drop_round(int n_rounds) { return (n_rounds / 2) > 1 ? (n_rounds / 2) : 1; }      // after this round the Huber kernel is off
LM_HD bool lm_round_exit(int n_edge, int num_good) { return n_edge < 4 || num_good < 4; }

// ---- one iteration: lambda_0, then the trials ----
LM_HD double lm_lambda_init(double max_abs_diag) { return 1e-5 * max_abs_diag; }                 // computeLambdaInit: tau * max |diag H|

// One iteration's trial loop: the gain ratio of the last trial, the trials counted so far (g2o's qmax) and whether lambda is still a number.
//     LmTrials tr;
//     do { <trial step>; if (!tr.verdict<..>(...)) { <pop the step>; if (!tr.lam_finite) break; } tr.count(); ++trials; } while (tr.another());
//     ++iterations; if (tr.terminate()) <the round's iterations end>;
struct LmTrials {
    double rho = 0;
    int qmax = 0;
    bool lam_finite = true;
    // The verdict on one trial step: accept (true: lambda shrinks, currentChi <- tempChi) or reject (lambda *= ni, ni doubles; the caller pops the step).
    // CUBE_POW: (2 rho - 1)^3 through pow() or as a product -- the two round differently on gfx950 and every caller keeps the form it was written with.
    template <bool CUBE_POW>
    LM_HD bool verdict(double& lambda, double& ni, double& currentChi, double tempChi, double scale) {
        rho = (currentChi - tempChi) / (scale + 1e-3);
        const bool accepted = rho > 0 && __builtin_isfinite(tempChi);
        if (accepted) {
            const double r21 = 2 * rho - 1;
            double alpha = 1. - (CUBE_POW ? pow(r21, 3.0) : r21 * r21 * r21);
            alpha = fmin(alpha, 2. / 3.);
            lambda *= fmax(1. / 3., alpha);
            ni = 2;
            currentChi = tempChi;
        } else {
            lambda *= ni;
            ni *= 2;
            if (!__builtin_isfinite(lambda)) lam_finite = false;
        }
        return accepted;
    }
    // A rejection that took lambda out of range (lam_finite false) ends the trial loop at once; every other trial is counted.  (Counting and the early
    // exit stay with the caller, inside its reject branch: folded into verdict() they cost lm_frame_kernel<16> and lm_kernel_big 16-32 bytes of scratch.)
    LM_HD void count() { ++qmax; }
    LM_HD bool another() const { return rho < 0 && qmax < LM_MAX_TRIALS; }
    LM_HD bool terminate() const { return qmax == LM_MAX_TRIALS || rho == 0 || !lam_finite; }      // of the round's iterations
};

// a failed solve's chi2: the trial is then rejected whatever the step
constexpr double LM_CHI2_FAILED = 1.7976931348623157e308;

// ---- the whole run, for a kernel that owns a problem from the first classification to the last ----
struct LmCounters {                                     // LmProblem::stats
    int rounds = 0, lm_its = 0, lm_trials = 0, num_good = 0;
    __device__ __forceinline__ void store(int* stats) const { stats[0] = rounds; stats[1] = lm_its; stats[2] = lm_trials; stats[3] = num_good; }
};
struct LmTrial { double chi, scale; bool ok; };         // what a trial step reports, already uniform over the workgroup

// Every value branched on here is uniform across the workgroup; the template adds no barrier, reduction or memory access of its own -- what a kernel
// needs of those lives in its callables:
//   initial() -> int                    the first classification; the inlier count the rounds start from
//   any_active() -> bool                g2o: nothing to optimise -> optimize() returns without iterating
//   linearise(robust_on, it, max_diag) -> double     chi2 at the standing state; at it == 0 also max |diag H| over the free vertices
//   trial(lambda, robust_on) -> LmTrial              solve, step (push), chi2 and step scale at the trial state
//   accept() / reject()                 keep the trial state / pop it
//   classify() -> int                   chi2 re-classification at the accepted state; the inlier count
// (taken by const reference: by value lm_frame_kernel<16> spilled 8 bytes per lane more)
template <bool CUBE_POW, class Problem, class Initial, class AnyActive, class Linearise, class Trial, class Accept, class Reject, class Classify>
__device__ __forceinline__ LmCounters lm_run_rounds(const Problem& P, const Initial& initial, const AnyActive& any_active, const Linearise& linearise, const Trial& trial,
                                                    const Accept& accept, const Reject& reject, const Classify& classify) {
    LmCounters n;
    n.num_good = initial();
    bool robust_on = true;
    const int drop = lm_drop_round(P.n_rounds);
    for (int round = 0; round < P.n_rounds; ++round) {
        if (lm_round_exit(P.n_edge, n.num_good)) break;
        ++n.rounds;
        const int iterations = any_active() ? P.its[round] : 0;
        double lambda = -1, ni = 2;
        for (int it = 0; it < iterations; ++it) {
            double max_diag = 0;
            double currentChi = linearise(robust_on, it, max_diag);
            if (it == 0) { lambda = lm_lambda_init(max_diag); ni = 2; }
            LmTrials tr;
            do {
                const LmTrial t = trial(lambda, robust_on);
                if (tr.template verdict<CUBE_POW>(lambda, ni, currentChi, t.ok ? t.chi : LM_CHI2_FAILED, t.scale)) accept();
                else { reject(); if (!tr.lam_finite) break; }
                tr.count();
                ++n.lm_trials;
            } while (tr.another());
            ++n.lm_its;
            if (tr.terminate()) break;
        }
        n.num_good = classify();
        if (round == drop) robust_on = false;
    }
    return n;
}

}  // namespace suo
