// ks_eval.h -- the arithmetic of the surrogate test-phase metrics (ks_eval_rows_device / ks_eval_fold_device, kspde.h):
// the per-row sums and the per-step tables of PDETrainingModule.test_step, one spelling for the kernels of ks_eval.hip
// (hipcc) and for the twin in ks_cpu.cpp (a plain C++ compiler).  The stencils are ks_internal.h's ref_point; nothing
// here is read by the stepper kernels.  Both builds use -ffp-contract=off: the inverse maps keep separately rounded steps.
#pragma once
#include "ks_internal.h"

namespace ks {

// Periodic index for |offset| <= n (the +-4 halo of the stencils on a row of n >= 4 points).
KS_HD int eval_wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

constexpr int EVAL_ROW_STATS = 18;   // KS_EVAL_ROW_STATS
constexpr int EVAL_TABLES = 25;      // KS_EVAL_TABLES

// ks_eval_batch plus the shape and the output, as the launch and the twin take them
struct EvalArgs {
    const float* truth;
    long truth_bs, truth_ts;
    const float* pred;
    long pred_bs, pred_ts;
    int pred_shift;
    const float* phi;
    int inv_kind;
    const float* inv_coef;
    float* truth_out;
    float* pred_out;
    int B, T, N;
    double* rowstats;
    Consts k;
};

// stransf.otransf.Inverse at column i in separately rounded fp32 steps (the library is built -ffp-contract=off):
// kind 1 ScaleTransform._affine with coef [4][N] = (a, b - a, d - c, c), kind 2 Normalize._inv with coef [2][N] = (s, m).
KS_HD float eval_inverse(int kind, const float* coef, int N, int i, float v) {
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

// The running sums of one (b, t) row (or of one lane's share of it).
struct EvalSums {
    enum { ERR = 0, RS = 4, RO = 7, DER = 10, COUNT = 22 };
    // ERR: sum|e|, sum e^2, sum|s|, sum s^2;  RS / RO: the reward sums of s / o -- (u_xx^2, u_x^2, u * phi) under
    // dissipation, (unused, unused, u^2) under l2control;  DER + 4 d: sum|ds - do|, sum (ds - do)^2, sum|ds|, sum ds^2 of
    // derivative d = u_x, u_xx, u_xxxx
    double v[COUNT];
};

// The share (first, first + step, ...) of row `row`: s the inverse-scaled truth, o the inverse-scaled prediction (with
// pred_shift the prediction of step 0 is the truth row itself, read through the same map), e = (float)(o - s).
template <class DIV, bool DISS>
KS_HD void eval_row_share(const EvalArgs& a, long row, int first, int step, EvalSums& sums) {
    const int N = a.N;
    const long b = row / a.T, t = row % a.T;
    const float* sr = a.truth + b * a.truth_bs + t * a.truth_ts;
    const float* pr = (a.pred_shift && t == 0) ? sr : a.pred + b * a.pred_bs + (t - (a.pred_shift ? 1 : 0)) * a.pred_ts;
    const float* fr = (DISS && a.phi) ? a.phi + row * N : nullptr;
    for (int i = first; i < N; i += step) {
        double ws[9], qs[9], wo[9], qo[9];
        float s = 0.0f, o = 0.0f;
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int m = -4; m <= 4; ++m) {
            const int j = eval_wrap(i + m, N);
            const float sv = eval_inverse(a.inv_kind, a.inv_coef, N, j, sr[j]);
            const float ov = eval_inverse(a.inv_kind, a.inv_coef, N, j, pr[j]);
            if (m == 0) {
                s = sv;
                o = ov;
            }
            ws[m + 4] = (double)sv;
            qs[m + 4] = ws[m + 4] * ws[m + 4];
            wo[m + 4] = (double)ov;
            qo[m + 4] = wo[m + 4] * wo[m + 4];
        }
        const int c = 4;
        if (a.truth_out) a.truth_out[row * N + i] = s;
        if (a.pred_out) a.pred_out[row * N + i] = o;
        const double e = (double)(o - s);   // the fp32 difference, as the reference forms it
        double* v = sums.v;
        v[EvalSums::ERR + 0] += std::fabs(e);
        v[EvalSums::ERR + 1] += e * e;
        v[EvalSums::ERR + 2] += std::fabs(ws[c]);
        v[EvalSums::ERR + 3] += qs[c];
        const RefPoint ps = ref_point<DIV>(ws, qs, c, 0.0, a.k), po = ref_point<DIV>(wo, qo, c, 0.0, a.k);
        if constexpr (DISS) {   // the sums of ks_reward_rows_kernel, in its order
            v[EvalSums::RS + 0] += ps.d2 * ps.d2;
            v[EvalSums::RS + 1] += ps.d1 * ps.d1;
            v[EvalSums::RO + 0] += po.d2 * po.d2;
            v[EvalSums::RO + 1] += po.d1 * po.d1;
            if (fr) {
                v[EvalSums::RS + 2] += ws[c] * (double)fr[i];
                v[EvalSums::RO + 2] += wo[c] * (double)fr[i];
            }
        } else {
            v[EvalSums::RS + 2] += qs[c];
            v[EvalSums::RO + 2] += qo[c];
        }
        const double ds[3] = {ps.d1, ps.d2, ps.d4}, dp[3] = {po.d1, po.d2, po.d4};
#ifdef __HIPCC__
#pragma unroll
#endif
        for (int d = 0; d < 3; ++d) {
            const double diff = ds[d] - dp[d];
            v[EvalSums::DER + 4 * d + 0] += std::fabs(diff);
            v[EvalSums::DER + 4 * d + 1] += diff * diff;
            v[EvalSums::DER + 4 * d + 2] += std::fabs(ds[d]);
            v[EvalSums::DER + 4 * d + 3] += ds[d] * ds[d];
        }
    }
}

// The 18 values of a row from its complete sums.  Rewards as ks_reward_rows_kernel forms them; under l2control rounded
// to fp32, the precision the reference's reward has there.
template <bool DISS>
KS_HD void eval_row_finish(const EvalSums& sums, int N, double* out) {
    const double* v = sums.v;
    for (int j = 0; j < 4; ++j) out[j] = v[EvalSums::ERR + j];
    for (int side = 0; side < 2; ++side) {
        const double* r = v + (side ? EvalSums::RO : EvalSums::RS);
        if constexpr (DISS)
            out[4 + side] = (-1.0) * ((r[0] / N + r[1] / N) + r[2] / N);
        else
            out[4 + side] = (double)(float)((-1.0) * (1.0 / N) * r[2]);
    }
    for (int j = 0; j < 12; ++j) out[6 + j] = v[EvalSums::DER + j];
}

// Output value i of the fold over rowstats [B][T][18]: i = 0 the MSE, i = 1 + k * T + t table k at step t, in the order
// of the dict test_step returns (training.py:254-270 of the reference): l1_loss, l2_loss, l1_loss_scaled,
// l2_loss_scaled, nrmse; the same five of the rewards (norms over the batch); then l1, l2, l1_scaled, l2_scaled, nrms
// of the derivatives, three tables each (u_x, u_xx, u_xxxx).  b runs in index order; a zero norm divides as IEEE does.
KS_HD double eval_fold_value(const double* st, int B, int T, int N, int i) {
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
    const int kind = k < 5 ? k : (k - 10) / 3, o = k < 5 ? 0 : 6 + 4 * ((k - 10) % 3);
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

#ifdef __HIPCC__
// ks_eval.hip: device pointers throughout
hipError_t launch_eval_rows(int objective, const EvalArgs& a, hipStream_t stream);
hipError_t launch_eval_fold(const double* rowstats, int B, int T, int N, double* tables, double* accum, hipStream_t stream);
#endif

}  // namespace ks
