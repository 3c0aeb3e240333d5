// bg_eval.h -- the arithmetic of the Burgers test-phase metrics (bg_eval_rows / bg_eval_fold / bg_derivatives,
// include/burgers/eval.h): the per-row sums and the per-step tables of PDETrainingModule.test_step on a Burgers env, one
// spelling that bg_eval.hip compiles for the device (the kernels) and for the host (the *_host entries).  The layout
// follows ks_eval.h; the stencils are those of include/burgers_hip.h taken in fp64 from the widened fp32 values; nothing
// here is read by the stepper kernels of burgers.hip.  Built with -ffp-contract=off: the inverse maps keep separately
// rounded steps, and the host and the device form every fp64 value by the same operations in the same order.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define BG_HD __host__ __device__ inline
#else
#define BG_HD inline
#endif

namespace bg {

constexpr int EVAL_ROW_STATS = 14;   // BG_EVAL_ROW_STATS
constexpr int EVAL_TABLES = 20;      // BG_EVAL_TABLES

// Periodic index for |offset| <= n (the +-2 halo of the stencils on a row of n >= 5 points).
BG_HD int eval_wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// bg_eval_batch plus the shape, the grid and the output, as the launch and the host entry take them
struct EvalArgs {
    const float* truth;
    long truth_bs, truth_ts;
    const float* pred;
    long pred_bs, pred_ts;
    int pred_shift;
    int inv_kind;
    const float* inv_coef;
    float* truth_out;
    float* pred_out;
    int B, T, N;
    double two_dx, twelve_dx2;   // 2 dx and 12 dx^2, one rounded product each
    double* rowstats;
};

// stransf.otransf.Inverse at column i in separately rounded fp32 steps: kind 1 ScaleTransform._affine with coef [4][N] =
// (a, b - a, d - c, c), kind 2 Normalize._inv with coef [2][N] = (s, m); eval_inverse of ks_eval.h.
BG_HD float eval_inverse(int kind, const float* coef, int N, int i, float v) {
    if (kind == 1) {
        float x = v - coef[i];
        x = x / coef[N + i];
        x = x * coef[2 * N + i];
        return x + coef[3 * N + i];
    }
    if (kind == 2) {
        const float x = v * coef[i];
        return x + coef[N + i];
    }
    return v;
}

// u_x = (u+1 - u-1) / (2 dx) and u_xx = (-u-2 + 16 u-1 - 30 u0 + 16 u+1 - u+2) / (12 dx^2) from the window w[0 .. 4] =
// u-2 .. u+2 in fp64.
BG_HD void derivatives(const double* w, double two_dx, double twelve_dx2, double& ux, double& uxx) {
    ux = (w[3] - w[1]) / two_dx;
    uxx = ((16.0 * (w[1] + w[3]) - (w[0] + w[4])) - 30.0 * w[2]) / twelve_dx2;
}

// The window of point i of an fp32 row of n points, widened.
BG_HD void window(const float* row, int n, int i, double* w) {
    for (int m = -2; m <= 2; ++m) w[m + 2] = (double)row[eval_wrap(i + m, n)];
}

// The running sums of one (b, t) row (or of one lane's share of it): 0-3 sum|e|, sum e^2, sum|s|, sum s^2; 4, 5 sum s^2 and
// sum o^2 (the reward sums); 6 + 4 d: sum|ds - do|, sum (ds - do)^2, sum|ds|, sum ds^2 of derivative d = u_x, u_xx.
struct EvalSums {
    enum { ERR = 0, REW = 4, DER = 6, COUNT = 14 };
    double v[COUNT];
};

// The share (first, first + step, ...) of row `row`: s the inverse-scaled truth, o the inverse-scaled prediction (with
// pred_shift the prediction of step 0 is the truth row itself, read through the same map), e = (float)(o - s).
BG_HD void eval_row_share(const EvalArgs& a, long row, int first, int step, EvalSums& sums) {
    const int N = a.N;
    const long b = row / a.T, t = row % a.T;
    const float* sr = a.truth + b * a.truth_bs + t * a.truth_ts;
    const float* pr = (a.pred_shift && t == 0) ? sr : a.pred + b * a.pred_bs + (t - (a.pred_shift ? 1 : 0)) * a.pred_ts;
    for (int i = first; i < N; i += step) {
        double ws[5], wo[5];
        float s = 0.0f, o = 0.0f;
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int m = -2; m <= 2; ++m) {
            const int j = eval_wrap(i + m, N);
            const float sv = eval_inverse(a.inv_kind, a.inv_coef, N, j, sr[j]);
            const float ov = eval_inverse(a.inv_kind, a.inv_coef, N, j, pr[j]);
            if (m == 0) {
                s = sv;
                o = ov;
            }
            ws[m + 2] = (double)sv;
            wo[m + 2] = (double)ov;
        }
        if (a.truth_out) a.truth_out[row * N + i] = s;
        if (a.pred_out) a.pred_out[row * N + i] = o;
        const double e = (double)(o - s);   // the fp32 difference, as the host lines form it
        double* v = sums.v;
        v[EvalSums::ERR + 0] += std::fabs(e);
        v[EvalSums::ERR + 1] += e * e;
        v[EvalSums::ERR + 2] += std::fabs(ws[2]);
        v[EvalSums::ERR + 3] += ws[2] * ws[2];
        v[EvalSums::REW + 0] += ws[2] * ws[2];
        v[EvalSums::REW + 1] += wo[2] * wo[2];
        double ds[2], dp[2];
        derivatives(ws, a.two_dx, a.twelve_dx2, ds[0], ds[1]);
        derivatives(wo, a.two_dx, a.twelve_dx2, dp[0], dp[1]);
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int d = 0; d < 2; ++d) {
            const double diff = ds[d] - dp[d];
            v[EvalSums::DER + 4 * d + 0] += std::fabs(diff);
            v[EvalSums::DER + 4 * d + 1] += diff * diff;
            v[EvalSums::DER + 4 * d + 2] += std::fabs(ds[d]);
            v[EvalSums::DER + 4 * d + 3] += ds[d] * ds[d];
        }
    }
}

// The 14 values of a row from its complete sums.  The rewards are the env's l2control reward_func rounded to fp32, the
// precision the host lines give it.
BG_HD void eval_row_finish(const EvalSums& sums, int N, double* out) {
    const double* v = sums.v;
    for (int j = 0; j < 4; ++j) out[j] = v[EvalSums::ERR + j];
    for (int side = 0; side < 2; ++side) out[4 + side] = (double)(float)((-1.0) * (1.0 / N) * v[EvalSums::REW + side]);
    for (int j = 0; j < 8; ++j) out[6 + j] = v[EvalSums::DER + j];
}

// Output value i of the fold over rowstats [B][T][14]: i = 0 the MSE, i = 1 + k * T + t table k at step t, in the order
// of the dict test_step returns when env.rhs hands out two derivatives: l1_loss, l2_loss, l1_loss_scaled,
// l2_loss_scaled, nrmse; the same five of the rewards (norms over the batch); then l1, l2, l1_scaled, l2_scaled, nrms
// of the derivatives, two tables each (u_x, u_xx).  b runs in index order; a zero norm divides as IEEE does.
BG_HD double eval_fold_value(const double* st, int B, int T, int N, int i) {
    constexpr int S = EVAL_ROW_STATS;
    if (i == 0) {
        double s = 0.0;
        for (long r = 0; r < (long)B * T; ++r) s += st[r * S + 1];
        return s / ((double)B * (double)T * (double)N);
    }
    const int k = (i - 1) / T, t = (i - 1) % T;
    if (k >= 5 && k < 10) {
        double e1 = 0.0, e2 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int b = 0; b < B; ++b) {
            const double* row = st + ((long)b * T + t) * S;
            const double r = row[4], d = r - row[5];
            e1 += std::fabs(d);
            e2 += d * d;
            r1 += std::fabs(r);
            r2 += r * r;
        }
        switch (k - 5) {
            case 0: return e1;
            case 1: return std::sqrt(e2);
            case 2: return e1 / r1;
            case 3: return std::sqrt(e2) / std::sqrt(r2);
            default: return e2 / r2;
        }
    }
    const int kind = k < 5 ? k : (k - 10) / 2, o = k < 5 ? 0 : 6 + 4 * ((k - 10) % 2);
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
        const double* row = st + ((long)b * T + t) * S + o;
        switch (kind) {
            case 0: s += row[0]; break;
            case 1: s += std::sqrt(row[1]); break;
            case 2: s += row[0] / row[2]; break;
            case 3: s += std::sqrt(row[1]) / std::sqrt(row[3]); break;
            default: s += row[1] / row[3]; break;
        }
    }
    return s / (double)B;
}

}  // namespace bg
