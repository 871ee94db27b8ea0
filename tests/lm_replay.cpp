// Replays scripted device results through the Levenberg controller (orb_slam3-1_amd/csrc/lm_control.h) the way
// lba_shard_optimize drives it with world size 1; tests/test_lm_control.py runs the same scripts through the Python driver.
//
// stdin, any number of scripts (numbers as C hex floats, %a):
//   script <max_iters> <lambda_init> <stop_at>   stop flag raised once <stop_at> trials ran (0: from the start, -1: never)
//   L <chi2> <max_diag_poses> <max_diag_landmarks>   the results of the linearisations, in order
//   T <solved> <chi2_new> <scale_poses> <scale_landmarks>   the results of the trials, in order
//   end
// stdout per script: "trial <accepted> <lambda after the trial>" per trial, then "stats <iterations> <trials> <stop_reason>
// <chi2_initial> <chi2_final> <lambda>", "trace <16 entries>" and "end".
// `lm_replay device` replays the scripts through the policy functions of the one-workgroup solvers instead
// (orb_slam3-1_amd/csrc/dense_lm_device.h, the loop of k_pose_opt / k_sim3_optimize) and appends rho to every trial line.
// `lm_replay flags <v>...` prints the trial status of each failure-flag value instead: solved, rejected or stalled.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dense_lm_device.h"
#include "lm_control.h"

namespace {

struct Lin { double chi, mdp, mdl; };
struct Trial { int solved; double chi, sp, sl; };

void replay(int max_iters, double lambda_init, long stop_at, const std::vector<Lin>& ls, const std::vector<Trial>& ts)
{
    lm::Levenberg c(max_iters);
    size_t li = 0, ti = 0;
    auto stop = [&]() { return stop_at >= 0 && (long)ti >= stop_at; };
    while (!c.capped()) {
        if (!c.begin_iteration(stop())) break;
        const Lin& l = ls.at(li++);
        c.linearized(l.chi, lm::initial_lambda(lambda_init, l.mdp, l.mdl));
        do {
            const Trial& t = ts.at(ti++);
            const bool accepted = c.trial(t.solved != 0, t.chi, t.sp + t.sl);
            std::printf("trial %d %a\n", accepted ? 1 : 0, c.lambda());
        } while (c.more_trials(stop()));
        if (!c.end_iteration()) break;
    }
    const LbaStats st = c.stats();
    std::printf("stats %d %d %d %a %a %a\ntrace", st.iterations, st.trials, st.stop_reason, st.chi2_initial, st.chi2_final, st.lambda);
    for (double v : st.chi2_trace) std::printf(" %a", v);
    std::printf("\nend\n");
}

// the loop of the kernels, plus what only the host drivers have: the user's lambda and the stop flag (stop reason 3)
void replay_device(int max_iters, double lambda_init, long stop_at, const std::vector<Lin>& ls, const std::vector<Trial>& ts)
{
    LbaStats st{};
    double lambda = -1.0, ni = 2, cur = 0, rho = 0;     // -1: lm::Levenberg's lambda before the first linearisation
    int nbad = 0;
    size_t li = 0, ti = 0;
    auto stop = [&]() { return stop_at >= 0 && (long)ti >= stop_at; };
    for (int it = 0; it < max_iters; it++) {
        if (stop()) { st.stop_reason = 3; break; }
        const Lin& l = ls.at(li++);
        cur = l.chi;
        const double ini = cur;
        if (it == 0) {
            const double Hu[3] = {l.mdp, 0.0, l.mdl};   // packed 2x2 with the two diagonal maxima
            st.chi2_initial = cur;
            lambda = lambda_init > 0 ? lambda_init : dlm::lambda_init<2>(Hu); ni = 2; nbad = 0;
        }
        int qmax = 0;
        rho = 0;
        do {
            const Trial& t = ts.at(ti++);
            const bool accepted = dlm::trial(t.solved != 0, t.chi, t.sp + t.sl, lambda, ni, cur, rho);
            qmax++;
            std::printf("trial %d %a %a\n", accepted ? 1 : 0, lambda, rho);
        } while (dlm::more_trials(rho, qmax) && !stop());
        st.iterations++; st.trials += qmax; st.chi2_final = cur;
        if (it < 16) st.chi2_trace[it] = cur;
        st.stop_reason = dlm::stop_reason(qmax, rho, ini, cur, nbad);
        if (st.stop_reason) break;
    }
    std::printf("stats %d %d %d %a %a %a\ntrace", st.iterations, st.trials, st.stop_reason, st.chi2_initial, st.chi2_final, lambda);
    for (double v : st.chi2_trace) std::printf(" %a", v);
    std::printf("\nend\n");
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "flags") == 0) {
        static const char* names[] = {"solved", "rejected", "stalled"};
        for (int i = 2; i < argc; i++) std::printf("%s\n", names[(int)lm::trial_status(std::strtod(argv[i], nullptr))]);
        return 0;
    }
    const bool device_form = argc > 1 && std::strcmp(argv[1], "device") == 0;
    int max_iters = 0;
    double lambda_init = 0;
    long stop_at = -1;
    std::vector<Lin> ls;
    std::vector<Trial> ts;
    char tag[16];
    while (std::scanf("%15s", tag) == 1) {
        const std::string k = tag;
        if (k == "script") {
            if (std::scanf("%d %lf %ld", &max_iters, &lambda_init, &stop_at) != 3) return 2;
            ls.clear();
            ts.clear();
        } else if (k == "L") {
            Lin l;
            if (std::scanf("%lf %lf %lf", &l.chi, &l.mdp, &l.mdl) != 3) return 2;
            ls.push_back(l);
        } else if (k == "T") {
            Trial t;
            if (std::scanf("%d %lf %lf %lf", &t.solved, &t.chi, &t.sp, &t.sl) != 4) return 2;
            ts.push_back(t);
        } else if (k == "end") {
            (device_form ? replay_device : replay)(max_iters, lambda_init, stop_at, ls, ts);
        } else {
            return 2;
        }
    }
    return 0;
}
