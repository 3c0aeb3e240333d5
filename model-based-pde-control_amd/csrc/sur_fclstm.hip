// sur_fclstm.hip -- whole-rollout kernels of the two fully-connected LSTM baselines (KSAutoRegFullyConnectedLSTM,
// KSLatentLSTM; pdecontrol/architectures): C ABI sur_fc_* in include/surrogate_hip.h, binding and autograd node in
// pdecontrol/surrogates/fclstm_hip.py.  A translation unit of its own, linked into libsurrogate_hip.so next to
// sur_kernels.hip (whose kernels it neither reads nor changes).
//
// The network is fixed: Linear 64 -> 32 -> 16 encoder, nn.LSTM(4, 16) on the 4 raw actuator values, Linear 16 -> 32 -> 64
// decoder; 6 672 fp32 parameters (26.7 KB) in named_parameters() order without the frozen H0 / C0.
//
// Forward (fc_fwd_kernel), ONE launch: a workgroup of 4 waves stages the weights in LDS once, TRANSPOSED ([in][out]),
// then every wave walks one sample through all K steps.  A matrix-vector product is "one lane per output row": lane r
// reads w[k * OUT + r] -- 64 consecutive words, one per bank -- and takes x[k] from lane k through v_readlane (an
// SGPR broadcast; no LDS traffic and no barrier for the vectors).  Layers narrower than the wave (32, 16 rows) are
// computed replicated, lane r holding row r mod OUT: replicated lanes read the same address (a broadcast, no conflict)
// and the next layer finds element k in lane k.  The 64 LSTM gate rows map one to one onto lanes (i, f, g, o quarters);
// the regrouping to 16-wide is four ds_bpermute.  Every sum is one fmaf chain in index order, starting from the bias.
//
// Backward (fc_bwd_kernel, fc_wgrad_kernel), TWO launches: the same wave-per-sample walk in reverse over the record the
// forward saved (256 floats per (sample, step): the pre-activations of the three hidden Linear layers, the gate
// activations, c', h', the running latent and the decoder output), weights in LDS in their own row-major layout (the
// transposed products read w[r * IN + lane]: consecutive again).  It writes the gradients of states, actions and c_in, and
// per (sample, step) one row of the workspace: the pre-activation gradients of the five matrix products and the four
// input rows the weight gradients need that are not kernel inputs.  fc_wgrad_kernel then sums the outer products: one
// thread per (parameter, quarter of the samples), samples and steps in index order, the four quarters added in order
// through LDS.  No floating-point atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/surrogate_hip.h"
#include "capi_error.h"

namespace {

constexpr int WAVE = 64, WAVES = 4, TPB = WAVE * WAVES;
constexpr int N = 64, E1 = 32, HID = 16, D1 = 32, NACT = 4, GATES = 4 * HID;
constexpr int FORM_AUTOREG = 0, FORM_LATENT = 1;
constexpr int ACT_SILU_TANH = 0, ACT_ELU_IDENTITY = 1;      // hidden activation, then the decoder's last activation

// ---- the flat parameter vector --------------------------------------------------------------------------------------
constexpr int P_W1 = 0, P_B1 = P_W1 + E1 * N, P_W2 = P_B1 + E1, P_B2 = P_W2 + HID * E1;
constexpr int P_WD1 = P_B2 + HID, P_BD1 = P_WD1 + D1 * HID, P_WD2 = P_BD1 + D1, P_BD2 = P_WD2 + N * D1;
constexpr int P_WIH = P_BD2 + N, P_WHH = P_WIH + GATES * NACT, P_BIH = P_WHH + GATES * HID, P_BHH = P_BIH + GATES;
constexpr int NPARAM = P_BHH + GATES;
static_assert(NPARAM == 6672, "parameter count of the fully-connected LSTM factories");

// ---- the record of one (sample, step) the forward saves -----------------------------------------------------------------
constexpr int R_Z1 = 0, R_Z2 = R_Z1 + E1, R_GATE = R_Z2 + HID, R_C = R_GATE + GATES, R_H = R_C + HID, R_ZLAT = R_H + HID;
constexpr int R_Z4 = R_ZLAT + HID, R_D2 = R_Z4 + D1, REC = R_D2 + N;
static_assert(REC == 256, "record size");
// ---- the workspace row of one (sample, step) the backward walk writes ---------------------------------------------------
constexpr int W_P1 = 0, W_P2 = W_P1 + E1, W_P3 = W_P2 + HID, W_P4 = W_P3 + GATES, W_P5 = W_P4 + D1;
constexpr int W_E1 = W_P5 + N, W_H = W_E1 + E1, W_DEC = W_H + HID, W_D1 = W_DEC + HID, ROW = W_D1 + D1;
static_assert(ROW == 304, "workspace row size");

// ---- activations ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int ACT>
__device__ __forceinline__ float hidden_act(float x)
{
    if (ACT == ACT_SILU_TANH) return x * sigmoidf_(x);
    return x > 0.0f ? x : expm1f(x);
}

// d activation / d input, from the pre-activation
template <int ACT>
__device__ __forceinline__ float hidden_slope(float x)
{
    if (ACT == ACT_SILU_TANH) {
        const float s = sigmoidf_(x);
        return s * fmaf(x, 1.0f - s, 1.0f);
    }
    return x > 0.0f ? 1.0f : expf(x);
}

template <int ACT>
__device__ __forceinline__ float last_act(float x) { return ACT == ACT_SILU_TANH ? tanhf(x) : x; }

// from the activation's output
template <int ACT>
__device__ __forceinline__ float last_slope(float y) { return ACT == ACT_SILU_TANH ? fmaf(-y, y, 1.0f) : 1.0f; }

// ---- matrix-vector products over the wave ---------------------------------------------------------------------------
// x[k] of lane k for every lane (k is a compile-time constant once the loops below are unrolled)
__device__ __forceinline__ float bcast(float v, int k)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// forward: wt is [IN][OUT] (transposed); returns row (lane mod OUT) of acc + W x, x[k] living in lane k
template <int IN, int OUT>
__device__ __forceinline__ float matvec(const float* wt, float acc, float x, int lane)
{
    const float* col = wt + (lane & (OUT - 1));
#pragma unroll
    for (int k = 0; k < IN; ++k) acc = fmaf(col[k * OUT], bcast(x, k), acc);
    return acc;
}

// backward: w is [OUT][IN] (row major); returns element (lane mod IN) of W^T p, p[r] living in lane r
template <int IN, int OUT>
__device__ __forceinline__ float matvec_t(const float* w, float p, int lane)
{
    const float* col = w + (lane & (IN - 1));
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < OUT; ++r) acc = fmaf(col[r * IN], bcast(p, r), acc);
    return acc;
}

// copies the flat parameters into LDS with every weight matrix transposed in place ([out][in] -> [in][out])
__device__ void stage_transposed(float* w, const float* __restrict__ P, int tid)
{
    for (int e = tid; e < NPARAM; e += TPB) {
        int off, in, out;
        if (e < P_B1) { off = P_W1; in = N; out = E1; }
        else if (e >= P_W2 && e < P_B2) { off = P_W2; in = E1; out = HID; }
        else if (e >= P_WD1 && e < P_BD1) { off = P_WD1; in = HID; out = D1; }
        else if (e >= P_WD2 && e < P_BD2) { off = P_WD2; in = D1; out = N; }
        else if (e >= P_WIH && e < P_WHH) { off = P_WIH; in = NACT; out = GATES; }
        else if (e >= P_WHH && e < P_BIH) { off = P_WHH; in = HID; out = GATES; }
        else { w[e] = P[e]; continue; }
        const int r = (e - off) / in, c = (e - off) % in;
        w[off + c * out + r] = P[e];
    }
}

// Linear 64 -> 32 -> 16 with the hidden activation; x[i] in lane i.  z1 in lane r mod 32, z2 in lane r mod 16.
template <int ACT>
__device__ __forceinline__ float encode(const float* w, float x, int lane, float& z1, float& z2)
{
    z1 = matvec<N, E1>(w + P_W1, w[P_B1 + (lane & (E1 - 1))], x, lane);
    z2 = matvec<E1, HID>(w + P_W2, w[P_B2 + (lane & (HID - 1))], hidden_act<ACT>(z1), lane);
    return hidden_act<ACT>(z2);
}

template <int FORM, int ACT>
__global__ void __launch_bounds__(TPB) fc_fwd_kernel(const float* __restrict__ P, int B, int S, int K, int su,
                                                     const float* __restrict__ states, const float* __restrict__ actions,
                                                     const float* __restrict__ c_in, float delta, float mul, float add,
                                                     float* __restrict__ outputs, float* __restrict__ deltas,
                                                     float* __restrict__ inlatents, float* __restrict__ outlatents,
                                                     float* __restrict__ h_out, float* __restrict__ c_out,
                                                     float* __restrict__ saved)
{
    __shared__ float w[NPARAM];
    stage_transposed(w, P, threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), j = lane & (HID - 1);
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                        // whole waves leave: the lanes of a working wave are all active

    float c = c_in ? c_in[(size_t)b * HID + j] : 0.0f;
    float h = 0.0f, z = 0.0f, out = 0.0f;      // h: the first step is always teacher forced (su >= 1)
    for (int k = 0; k < K; ++k) {
        const size_t step = (size_t)b * K + k;
        const bool given = k < su;             // wave uniform
        const float a = actions[step * NACT + (lane & (NACT - 1))];
        float x = 0.0f, z1 = 0.0f, z2 = 0.0f, inl = 0.0f;
        if (given) {
            x = states[((size_t)b * S + k) * N + lane];
            h = inl = encode<ACT>(w, x, lane, z1, z2);
            if (FORM == FORM_LATENT && k == 0) z = h;
        } else if (FORM == FORM_LATENT) {
            inl = z;
        } else if (inlatents) {                // the re-encoded prediction: reported, never read
            float t1, t2;
            inl = encode<ACT>(w, out, lane, t1, t2);
        }
        if (inlatents && lane < HID) inlatents[step * HID + lane] = inl;

        float pre = w[P_BIH + lane] + w[P_BHH + lane];
        pre = matvec<NACT, GATES>(w + P_WIH, pre, a, lane);
        pre = matvec<HID, GATES>(w + P_WHH, pre, h, lane);
        const float gate = (lane >> 4) == 2 ? tanhf(pre) : sigmoidf_(pre);
        const float gi = __shfl(gate, j), gf = __shfl(gate, HID + j), gg = __shfl(gate, 2 * HID + j),
                    go = __shfl(gate, 3 * HID + j);
        c = fmaf(gf, c, gi * gg);
        h = go * tanhf(c);
        if (FORM == FORM_LATENT) z = fmaf(delta, h, z);

        const float z4 = matvec<HID, D1>(w + P_WD1, w[P_BD1 + (lane & (D1 - 1))], FORM == FORM_LATENT ? z : h, lane);
        const float d2 = last_act<ACT>(matvec<D1, N>(w + P_WD2, w[P_BD2 + lane], hidden_act<ACT>(z4), lane));
        if (FORM == FORM_LATENT) {
            out = d2;
        } else {
            deltas[step * N + lane] = d2;
            out = fmaf(delta, fmaf(mul, d2, add), given ? x : out);
        }
        outputs[step * N + lane] = out;
        if (lane < HID) outlatents[step * HID + lane] = h;
        if (saved) {
            float* rec = saved + step * REC;
            if (lane < E1) rec[R_Z1 + lane] = z1;
            if (lane < HID) {
                rec[R_Z2 + lane] = z2;
                rec[R_C + lane] = c;
                rec[R_H + lane] = h;
                rec[R_ZLAT + lane] = z;
            }
            rec[R_GATE + lane] = gate;
            if (lane < D1) rec[R_Z4 + lane] = z4;
            rec[R_D2 + lane] = d2;
        }
    }
    if (lane < HID) {
        h_out[(size_t)b * HID + lane] = h;
        c_out[(size_t)b * HID + lane] = c;
    }
}

template <int FORM, int ACT>
__global__ void __launch_bounds__(TPB) fc_bwd_kernel(const float* __restrict__ P, int B, int S, int K, int su,
                                                     const float* __restrict__ c_in, const float* __restrict__ saved,
                                                     float delta, float mul, const float* __restrict__ d_out,
                                                     const float* __restrict__ d_del, const float* __restrict__ d_inl,
                                                     const float* __restrict__ d_outl, const float* __restrict__ d_h_out,
                                                     const float* __restrict__ d_c_out, float* __restrict__ d_states,
                                                     float* __restrict__ d_actions, float* __restrict__ d_h_in,
                                                     float* __restrict__ d_c_in, float* __restrict__ work)
{
    __shared__ float w[NPARAM];
    for (int e = threadIdx.x; e < NPARAM; e += TPB) w[e] = P[e];
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), j = lane & (HID - 1), m = lane & (E1 - 1);
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= B) return;

    float g = 0.0f;                                                   // d output_k, lane = grid point (autoregressive form)
    float dh_carry = d_h_out ? d_h_out[(size_t)b * HID + j] : 0.0f;   // d h'_k from the step after it
    float dc_carry = d_c_out ? d_c_out[(size_t)b * HID + j] : 0.0f;
    float dz_carry = 0.0f;                                            // latent form: d z_{k+1} from the steps after k
    for (int k = K - 1; k >= 0; --k) {
        const size_t step = (size_t)b * K + k;
        const bool given = k < su;
        const float* rec = saved + step * REC;
        float* row = work + step * ROW;
        const float z1 = rec[R_Z1 + m], z2 = rec[R_Z2 + j], z4 = rec[R_Z4 + m], d2 = rec[R_D2 + lane];
        const float gi = rec[R_GATE + j], gf = rec[R_GATE + HID + j], gg = rec[R_GATE + 2 * HID + j],
                    go = rec[R_GATE + 3 * HID + j];
        const float c_new = rec[R_C + j];
        const float c_prev = k > 0 ? rec[R_C + j - REC] : (c_in ? c_in[(size_t)b * HID + j] : 0.0f);

        // decoder
        float dd2 = d_out ? d_out[step * N + lane] : 0.0f;
        if (FORM == FORM_AUTOREG) {
            g = dd2 + ((k + 1 < K && k + 1 >= su) ? g : 0.0f);       // step k + 1 integrates from output_k when free running
            dd2 = fmaf(delta * mul, g, d_del ? d_del[step * N + lane] : 0.0f);
        }
        const float p5 = dd2 * last_slope<ACT>(d2);
        const float p4 = matvec_t<D1, N>(w + P_WD2, p5, lane) * hidden_slope<ACT>(z4);
        float dh = matvec_t<HID, D1>(w + P_WD1, p4, lane) + dz_carry;   // d (decoder input); dz_carry is 0 in the autoreg form
        if (FORM == FORM_LATENT) {
            dz_carry = dh + ((!given && d_inl) ? d_inl[step * HID + j] : 0.0f);   // z_k is inlatents[k] when free running
            dh *= delta;
        }
        dh += (d_outl ? d_outl[step * HID + j] : 0.0f) + dh_carry;
        row[W_P5 + lane] = p5;
        if (lane < D1) {
            row[W_P4 + lane] = p4;
            row[W_D1 + lane] = hidden_act<ACT>(z4);
        }
        if (lane < HID) row[W_DEC + lane] = rec[(FORM == FORM_LATENT ? R_ZLAT : R_H) + lane];

        // LSTM cell
        const float tc = tanhf(c_new);
        const float dc = fmaf(dh * go, fmaf(-tc, tc, 1.0f), dc_carry);
        dc_carry = dc * gf;
        const int q = lane >> 4;
        const float p3 = q == 0 ? dc * gg * gi * (1.0f - gi)
                       : q == 1 ? dc * c_prev * gf * (1.0f - gf)
                       : q == 2 ? dc * gi * fmaf(-gg, gg, 1.0f)
                                : dh * tc * go * (1.0f - go);
        row[W_P3 + lane] = p3;
        const float dH = matvec_t<HID, GATES>(w + P_WHH, p3, lane);
        const float da = matvec_t<NACT, GATES>(w + P_WIH, p3, lane);
        if (d_actions && lane < NACT) d_actions[step * NACT + lane] = da;

        if (given) {                          // H was the encoded given state
            float de2 = dH + (d_inl ? d_inl[step * HID + j] : 0.0f);
            if (FORM == FORM_LATENT && k == 0) de2 += dz_carry;      // z_0 is the encoded first state
            const float p2 = de2 * hidden_slope<ACT>(z2);
            const float p1 = matvec_t<E1, HID>(w + P_W2, p2, lane) * hidden_slope<ACT>(z1);
            const float dx = matvec_t<N, E1>(w + P_W1, p1, lane);
            if (lane < HID) {
                row[W_P2 + lane] = p2;
                row[W_H + lane] = hidden_act<ACT>(z2);
            }
            if (lane < E1) {
                row[W_P1 + lane] = p1;
                row[W_E1 + lane] = hidden_act<ACT>(z1);
            }
            if (d_states) d_states[((size_t)b * S + k) * N + lane] = FORM == FORM_AUTOREG ? dx + g : dx;
            dh_carry = 0.0f;
        } else {                              // H was h' of step k - 1 (k >= su >= 1)
            if (lane < HID) row[W_H + lane] = rec[R_H + lane - REC];
            dh_carry = dH;
        }
    }
    if (d_states)
        for (int e = lane; e < (S - su) * N; e += WAVE) d_states[((size_t)b * S + su) * N + e] = 0.0f;
    if (lane < HID) {
        if (d_c_in) d_c_in[(size_t)b * HID + lane] = dc_carry;
        if (d_h_in) d_h_in[(size_t)b * HID + lane] = 0.0f;            // the first step replaces H: no path from h_in
    }
}

// d_params[p] = sum over samples and steps of (pre-activation gradient row) x (input row), one thread per (parameter,
// quarter of the samples): quarter s takes samples s, s + 4, ...; steps in order; then ((q0 + q1) + q2) + q3.
constexpr int WG_PARAMS = 64, WG_SLICES = TPB / WG_PARAMS;
constexpr int SRC_ONE = 0, SRC_WORK = 1, SRC_STATES = 2, SRC_ACTIONS = 3;

__global__ void __launch_bounds__(TPB) fc_wgrad_kernel(int B, int S, int K, int su, const float* __restrict__ states,
                                                       const float* __restrict__ actions, const float* __restrict__ work,
                                                       float* __restrict__ d_params)
{
    __shared__ float part[WG_SLICES][WG_PARAMS];
    const int t = threadIdx.x & (WG_PARAMS - 1), slice = threadIdx.x / WG_PARAMS;
    const int p = blockIdx.x * WG_PARAMS + t;
    float acc = 0.0f;
    if (p < NPARAM) {
        // where the parameter's two factors live: p_off in the workspace row, the input by source and column
        int p_off, src = SRC_ONE, col = 0, steps = K;
        if (p < P_B1) { p_off = W_P1 + p / N; src = SRC_STATES; col = p % N; steps = su; }
        else if (p < P_W2) { p_off = W_P1 + p - P_B1; steps = su; }
        else if (p < P_B2) { p_off = W_P2 + (p - P_W2) / E1; src = SRC_WORK; col = W_E1 + (p - P_W2) % E1; steps = su; }
        else if (p < P_WD1) { p_off = W_P2 + p - P_B2; steps = su; }
        else if (p < P_BD1) { p_off = W_P4 + (p - P_WD1) / HID; src = SRC_WORK; col = W_DEC + (p - P_WD1) % HID; }
        else if (p < P_WD2) { p_off = W_P4 + p - P_BD1; }
        else if (p < P_BD2) { p_off = W_P5 + (p - P_WD2) / D1; src = SRC_WORK; col = W_D1 + (p - P_WD2) % D1; }
        else if (p < P_WIH) { p_off = W_P5 + p - P_BD2; }
        else if (p < P_WHH) { p_off = W_P3 + (p - P_WIH) / NACT; src = SRC_ACTIONS; col = (p - P_WIH) % NACT; }
        else if (p < P_BIH) { p_off = W_P3 + (p - P_WHH) / HID; src = SRC_WORK; col = W_H + (p - P_WHH) % HID; }
        else if (p < P_BHH) { p_off = W_P3 + p - P_BIH; }
        else { p_off = W_P3 + p - P_BHH; }
        for (int b = slice; b < B; b += WG_SLICES) {
            const float* row = work + (size_t)b * K * ROW;
            const float* in = src == SRC_STATES ? states + (size_t)b * S * N + col
                            : src == SRC_ACTIONS ? actions + (size_t)b * K * NACT + col : row + col;
            const int stride = src == SRC_STATES ? N : src == SRC_ACTIONS ? NACT : ROW;
            if (src == SRC_ONE) {
                for (int k = 0; k < steps; ++k) acc += row[(size_t)k * ROW + p_off];
            } else {
                for (int k = 0; k < steps; ++k) acc = fmaf(row[(size_t)k * ROW + p_off], in[(size_t)k * stride], acc);
            }
        }
    }
    part[slice][t] = acc;
    __syncthreads();
    if (slice == 0 && p < NPARAM) {
        float s = part[0][t];
        for (int q = 1; q < WG_SLICES; ++q) s += part[q][t];
        d_params[p] = s;
    }
}

// capi_error.h's fail(), written into the buffer sur_last_error() hands out: sur_kernels.hip owns that one (the header
// gives every translation unit a thread-local g_err of its own; both are sizeof(g_err) bytes)
__attribute__((format(printf, 2, 3))) int fc_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(const_cast<char*>(sur_last_error()), sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int fc_launch_status(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fc_fail(-2, "%s launch failed: %s", who, hipGetErrorString(e));
}

bool known(int form, int act)
{
    return (form == FORM_AUTOREG || form == FORM_LATENT) && (act == ACT_SILU_TANH || act == ACT_ELU_IDENTITY);
}

}  // namespace

extern "C" {

int sur_fc_param_count(void) { return NPARAM; }

int sur_fc_supported(int n, int enc_mid, int latent, int dec_mid, int actions, int form, int act, int nparams)
{
    if (n != N) return fc_fail(-4, "sur_fc_supported: grid width %d (the kernels are built for N = %d)", n, N);
    if (enc_mid != E1 || latent != HID || dec_mid != D1)
        return fc_fail(-4, "sur_fc_supported: layers 64 -> %d -> %d -> %d -> 64 (the kernels take 64 -> 32 -> 16 -> 32 -> 64)",
                       enc_mid, latent, dec_mid);
    if (actions != NACT) return fc_fail(-4, "sur_fc_supported: %d actuator values (the kernels take %d)", actions, NACT);
    if (!known(form, act)) return fc_fail(-4, "sur_fc_supported: unknown form %d or activation set %d", form, act);
    if (nparams != NPARAM) return fc_fail(-4, "sur_fc_supported: %d parameters (the kernels take %d)", nparams, NPARAM);
    return 0;
}

long sur_fc_saved_floats(int B, int K) { return B > 0 && K > 0 ? (long)B * K * REC : 0; }

long sur_fc_workspace_floats(int B, int K) { return B > 0 && K > 0 ? (long)B * K * ROW : 0; }

int sur_fc_forward(void* stream, const float* params, int form, int act, int B, int S, int K, const float* states,
                   const float* actions, const float* h_in, const float* c_in, float delta, float mul, float add,
                   float* outputs, float* deltas, float* inlatents, float* outlatents, float* h_out, float* c_out,
                   float* saved)
{
    (void)h_in;                                 // the first step is teacher forced: H is replaced before it is read
    if (!params || !states || !actions || !outputs || !outlatents || !h_out || !c_out)
        return fc_fail(-1, "sur_fc_forward: a required pointer is NULL");
    if (B <= 0 || S <= 0 || K <= 0) return fc_fail(-1, "sur_fc_forward: B = %d, S = %d, K = %d must be positive", B, S, K);
    if (!known(form, act)) return fc_fail(-1, "sur_fc_forward: unknown form %d or activation set %d", form, act);
    if (form == FORM_AUTOREG && !deltas) return fc_fail(-1, "sur_fc_forward: the autoregressive form writes deltas");
    const int su = S < K ? S : K;
    const dim3 grid((B + WAVES - 1) / WAVES), block(TPB);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define FC_FWD(F, A)                                                                                                     \
    hipLaunchKernelGGL((fc_fwd_kernel<F, A>), grid, block, 0, st, params, B, S, K, su, states, actions, c_in, delta, mul, \
                       add, outputs, deltas, inlatents, outlatents, h_out, c_out, saved)
    if (form == FORM_AUTOREG) {
        if (act == ACT_SILU_TANH) FC_FWD(FORM_AUTOREG, ACT_SILU_TANH); else FC_FWD(FORM_AUTOREG, ACT_ELU_IDENTITY);
    } else {
        if (act == ACT_SILU_TANH) FC_FWD(FORM_LATENT, ACT_SILU_TANH); else FC_FWD(FORM_LATENT, ACT_ELU_IDENTITY);
    }
#undef FC_FWD
    return fc_launch_status("sur_fc_forward");
}

int sur_fc_backward(void* stream, const float* params, int form, int act, int B, int S, int K, const float* states,
                    const float* actions, const float* c_in, const float* saved, float delta, float mul,
                    const float* d_outputs, const float* d_deltas, const float* d_inlatents, const float* d_outlatents,
                    const float* d_h_out, const float* d_c_out, float* d_states, float* d_actions, float* d_h_in,
                    float* d_c_in, float* d_params, float* work)
{
    if (!params || !states || !actions || !saved) return fc_fail(-1, "sur_fc_backward: a required pointer is NULL");
    if (!work) return fc_fail(-1, "sur_fc_backward: no workspace (sur_fc_workspace_floats(B, K) floats)");
    if (B <= 0 || S <= 0 || K <= 0) return fc_fail(-1, "sur_fc_backward: B = %d, S = %d, K = %d must be positive", B, S, K);
    if (!known(form, act)) return fc_fail(-1, "sur_fc_backward: unknown form %d or activation set %d", form, act);
    const int su = S < K ? S : K;
    const dim3 grid((B + WAVES - 1) / WAVES), block(TPB);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define FC_BWD(F, A)                                                                                                     \
    hipLaunchKernelGGL((fc_bwd_kernel<F, A>), grid, block, 0, st, params, B, S, K, su, c_in, saved, delta, mul, d_outputs, \
                       d_deltas, d_inlatents, d_outlatents, d_h_out, d_c_out, d_states, d_actions, d_h_in, d_c_in, work)
    if (form == FORM_AUTOREG) {
        if (act == ACT_SILU_TANH) FC_BWD(FORM_AUTOREG, ACT_SILU_TANH); else FC_BWD(FORM_AUTOREG, ACT_ELU_IDENTITY);
    } else {
        if (act == ACT_SILU_TANH) FC_BWD(FORM_LATENT, ACT_SILU_TANH); else FC_BWD(FORM_LATENT, ACT_ELU_IDENTITY);
    }
#undef FC_BWD
    const int rc = fc_launch_status("sur_fc_backward");
    if (rc || !d_params) return rc;
    hipLaunchKernelGGL(fc_wgrad_kernel, dim3((NPARAM + WG_PARAMS - 1) / WG_PARAMS), block, 0, st, B, S, K, su, states, actions,
                       work, d_params);
    return fc_launch_status("sur_fc_backward (weight gradients)");
}

}  // extern "C"
