// Levenberg-Marquardt policy of g2o, host side and device free: OptimizationAlgorithmLevenberg::solve
// (optimization_algorithm_levenberg.cpp:61-169) inside SparseOptimizer::optimize (sparse_optimizer.cpp:395-414).
// One controller per problem; its steps are the points where a driver waits for the device:
//   begin_iteration -> linearized -> trial [-> trial ...] while more_trials -> end_iteration -> begin_iteration ...
// The drivers (lba_shard_optimize, lba_solve_batch, liba_run) keep the device choreography: which state is accepted, which errors
// are current, lambda hints, launch flags, sequence numbers.  Plain C++17: g++ compiles it on its own (tests/test_lm_control.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/orbslam3_hip.h"

namespace lm {

// The factorisation's published failure flag (device scalar [5]): 0 solved, 1 a pivot block was not positive definite (the trial
// is rejected), 2 a bounded spin wait between workgroups expired (flow_wait): a hang-class event, an error and never a rejected trial.
enum class TrialStatus { kSolved, kNotPositiveDefinite, kStalled };
inline TrialStatus trial_status(double failure_flag)
{
    if (failure_flag == 0.0) return TrialStatus::kSolved;
    return failure_flag == 2.0 ? TrialStatus::kStalled : TrialStatus::kNotPositiveDefinite;
}

// computeLambdaInit (levenberg.cpp:171-185) of the LocalBA drivers: the user's lambda, else tau * max(diag H) with tau = 1e-5
inline double initial_lambda(double lambda_init, double max_diag_poses, double max_diag_landmarks)
{
    return lambda_init > 0 ? lambda_init : 1e-5 * std::max(max_diag_poses, max_diag_landmarks);
}

class Levenberg {
public:
    enum Step { kBegin, kLinearize, kTrial, kDone };

    explicit Levenberg(int max_iters, double lambda = -1.0) : max_iters_(max_iters), lambda_(lambda) {}

    Step step() const { return step_; }
    int iteration() const { return it_; }
    double lambda() const { return lambda_; }
    double chi2() const { return chi_; }
    bool capped() const { return it_ >= max_iters_; }

    // false (and done) when max_iters iterations ran or, below that cap, when `stop` (the caller's stop flag) is raised: stop reason 3
    bool begin_iteration(bool stop)
    {
        if (capped()) { step_ = kDone; return false; }
        if (stop) { st_.stop_reason = 3; step_ = kDone; return false; }
        step_ = kLinearize;
        return true;
    }

    // chi2 of the linearised estimate; on the first iteration also lambda := lambda0 (read there only), nu := 2, nBad := 0
    void linearized(double chi2, double lambda0)
    {
        chi_ = ini_chi_ = chi2;
        if (it_ == 0) { st_.chi2_initial = chi2; lambda_ = lambda0; ni_ = 2; n_bad_ = 0; }
        rho_ = 0;
        qmax_ = 0;
        step_ = kTrial;
    }

    // one trial at lambda(): its chi2, the scale dx^T (lambda dx + b) summed over all parts, and whether the system was solved.
    // Returns true when the trial state is accepted (discardTop), false when the old state is kept (pop).
    bool trial(bool solved, double chi2_new, double scale)
    {
        const double temp_chi = solved ? chi2_new : std::numeric_limits<double>::max();
        rho_ = (chi_ - temp_chi) / (scale + 1e-3);
        const bool accept = rho_ > 0 && std::isfinite(temp_chi);
        if (accept) {
            double alpha = 1. - std::pow((2 * rho_ - 1), 3);
            alpha = std::min(alpha, 2. / 3.);
            lambda_ *= std::max(1. / 3., alpha);
            ni_ = 2;
            chi_ = temp_chi;
        } else {
            lambda_ *= ni_;
            ni_ *= 2;
        }
        qmax_++;
        st_.trials++;
        return accept;
    }

    // another trial in this iteration?  `stop`: the caller's stop flag, polled after every trial
    bool more_trials(bool stop) const { return rho_ < 0 && qmax_ < 10 && !stop; }

    // chi2 trace, then stop reasons 1 (ten trials or rho == 0) and 2 (three iterations in a row below 1e-3 relative gain).
    // Returns false (and done) on a stop.
    bool end_iteration()
    {
        st_.iterations++;
        if (it_ < 16) st_.chi2_trace[it_] = chi_;
        st_.chi2_final = chi_;
        step_ = kDone;
        if (qmax_ == 10 || rho_ == 0) { st_.stop_reason = 1; return false; }
        if ((ini_chi_ - chi_) * 1e3 < ini_chi_) n_bad_++; else n_bad_ = 0;
        if (n_bad_ >= 3) { st_.stop_reason = 2; return false; }
        it_++;
        step_ = kBegin;
        return true;
    }

    LbaStats stats() const
    {
        LbaStats s = st_;
        s.lambda = lambda_;
        return s;
    }

private:
    int max_iters_;
    double lambda_;
    double ni_ = 2, rho_ = 0, chi_ = 0, ini_chi_ = 0;
    int n_bad_ = 0, it_ = 0, qmax_ = 0;
    Step step_ = kBegin;
    LbaStats st_{};
};

}  // namespace lm
