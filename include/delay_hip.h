/*
 * delay_hip.h -- C ABI of libdelay_hip.so: whole-rollout gfx950 kernels of the delay-embedding CNN surrogate
 * (KSDelayCNNSurrogateFactory, pdecontrol/architectures/delay.py; DelayTransitionModel, pdecontrol/surrogates/transition.py).
 *
 * The network is fixed: N = 64, a 3-block residual encoder to 8 x 8, a 2-layer action encoder 4 -> 4 x 8, a window of
 * delay = 3 (state, action) encodings, an MLP 288 -> 96 -> 64 -> 64 and a transposed-convolution decoder back to 64.
 * All parameters travel as ONE flat fp32 vector in the module's named_parameters() order (dly_param_count() floats).
 *
 *   dly_forward    one launch per rollout call: one workgroup per sample runs every step (teacher forcing on the first
 *                  min(S, K) given states, then free running on the re-encoded prediction).  The context window is a
 *                  3-slot ring in LDS.  Writes outputs, deltas (decoder outputs), inlatents (the encoded state each step
 *                  appended), outlatents (MLP outputs) and the final context.  Nothing else is saved: the backward
 *                  recomputes from inlatents / outlatents and the inputs.
 *   dly_backward   two launches: one workgroup per sample walks the steps backwards (integration chain, decoder, MLP,
 *                  the window's slot gradients, encoder and action-encoder backward) and adds the parameter gradients
 *                  into its own row of `work`; a second kernel sums the rows in sample order.  No atomics: the same
 *                  inputs give bit-identical gradients.
 *
 * Layouts (contiguous fp32, DEVICE pointers): states [B][S][64]; actions [B][K][4] (already mapped to the K internal
 * steps); context S [B][3][8][8], A [B][3][4][8], oldest slot first; outputs, deltas, inlatents, outlatents [B][K][64].
 * dscaling is affine: dscaling(d) = d * mul + add.  Optional pointers may be NULL (a NULL context is zero; a NULL
 * gradient input is zero; a NULL gradient output is not written).  Everything is enqueued on `stream`: no host
 * synchronisation, no device allocation.  Return 0 on success, negative on error (dly_last_error()).
 */
#ifndef DELAY_HIP_H
#define DELAY_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* number of floats of the flat parameter vector (39 830) */
int dly_param_count(void);

/* 0 when the kernels implement this layout, else a negative code with the reason in dly_last_error() */
int dly_supported(int n, int delay, int schannels, int ssize, int achannels, int asize, int actions, int nparams);

/* floats of the `work` buffer dly_backward needs for batch B */
long dly_workspace_floats(int B);

int dly_forward(void* stream, const float* params, int B, int S, int K, const float* states, const float* actions,
                const float* ctx_s_in, const float* ctx_a_in, float delta, float mul, float add,
                float* outputs, float* deltas, float* inlatents, float* outlatents, float* ctx_s_out, float* ctx_a_out);

int dly_backward(void* stream, const float* params, int B, int S, int K, const float* states, const float* actions,
                 const float* ctx_s_in, const float* ctx_a_in, const float* inlatents, const float* outlatents,
                 float delta, float mul,
                 const float* d_outputs, const float* d_deltas, const float* d_inlatents, const float* d_outlatents,
                 const float* d_ctx_s_out, const float* d_ctx_a_out,
                 float* d_states, float* d_actions, float* d_ctx_s_in, float* d_ctx_a_in, float* d_params, float* work);

const char* dly_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
