/*
 * surrogate_hip.h -- C ABI of libsurrogate_hip.so: fused gfx950 kernels for the surrogate's TBPTT step.
 *
 * The reference runs the surrogate as ~60 tiny torch CPU ops per time step
 * (pdecontrol/surrogates/surrogate.py:97-119 -> transition.py:218-226 + models/cnn.py:126-145,35-70).
 * On an MI355X that shape is launch-latency bound, so whole modules are fused per sample:
 *
 *   sur_encoder_forward / _backward   3 x ResidualBlock (models/cnn.py:73-145) as built by
 *                                     architectures/autoreg.py:51-73: [M,1,N] -> [M,C3,N/4]
 *   sur_chunk_forward / _backward     a whole TBPTT chunk of K rollout steps (surrogate.py:97-119):
 *                                     per step CNNLSTMCell (transition.py:218-226) + state decoder
 *                                     (autoreg.py:79-94) + integration out = base + delta*(d*mul+add);
 *                                     teacher forcing on the first S steps (transition.py:274-279),
 *                                     free running afterwards (:285-296).  Only the cell is a recurrence: its
 *                                     time loop runs INSIDE one kernel (weights and hidden state in LDS, one
 *                                     workgroup per sample); the decoders of all (step, sample) pairs run in
 *                                     parallel on every CU, forward and backward.
 *   sur_flush_*_grads                 reduces the per-workgroup partial gradient rows into the
 *                                     parameter gradient tensors (deterministic, no atomics)
 *
 * One workgroup handles one sample (or one (step, sample) pair) at a time with every activation in LDS; forward
 * launches can save their intermediates (`saved` buffers) and the backward launches read them back instead of
 * recomputing.  Parameter gradients are summed over space and time inside the workgroup and added to that
 * workgroup's own row of `partial` ([rows][sum(size)] fp32, caller-allocated, zero-initialised); the flush
 * kernels sum the rows into g[] (optionally applying the Adam update, `sur_adam`) and re-zero them.
 *
 * All pointers are DEVICE pointers of contiguous fp32 tensors; launches are asynchronous on the
 * given hipStream_t.  Return 0 on success, negative on error (sur_last_error()).
 */
#ifndef SURROGATE_HIP_H
#define SURROGATE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* parameter order inside one ResidualBlock */
enum { SUR_RB_CONV1 = 0, SUR_RB_LN1_W, SUR_RB_LN1_B, SUR_RB_CONV2, SUR_RB_LN2_W, SUR_RB_LN2_B, SUR_RB_SKIP,
       SUR_RB_LN3_W, SUR_RB_LN3_B, SUR_RB_NPARAM };
#define SUR_ENC_NPARAM (3 * SUR_RB_NPARAM)

typedef struct sur_encoder_params {
    const float* w[SUR_ENC_NPARAM]; /* weights, block-major                                     */
    float* g[SUR_ENC_NPARAM];       /* gradient tensors (targets of sur_flush_encoder_grads)    */
    int size[SUR_ENC_NPARAM];       /* element count of each parameter                           */
    int c[4];                       /* channels: in, block0, block1, block2 (1,8,16,16)          */
    int stride[3];                  /* 2, 2, 1                                                   */
    int n;                          /* input width N                                             */
    float* partial;                 /* [rows][sum(size)] partial gradient rows                   */
    int rows;
} sur_encoder_params;

/* parameter order of the chunk kernel */
enum { SUR_ST_WXI = 0, SUR_ST_BXI, SUR_ST_WHI, SUR_ST_WXF, SUR_ST_BXF, SUR_ST_WHF, SUR_ST_WXC, SUR_ST_BXC,
       SUR_ST_WHC, SUR_ST_WXO, SUR_ST_BXO, SUR_ST_WHO,
       SUR_ST_DC0_W, SUR_ST_DC0_B, SUR_ST_LN0_W, SUR_ST_LN0_B, SUR_ST_DC1_W, SUR_ST_DC1_B, SUR_ST_LN1_W,
       SUR_ST_LN1_B, SUR_ST_CV2_W, SUR_ST_CV2_B, SUR_ST_LN2_W, SUR_ST_LN2_B, SUR_ST_CV3_W, SUR_ST_CV3_B,
       SUR_ST_NPARAM };

typedef struct sur_chunk_params {
    const float* w[SUR_ST_NPARAM];
    float* g[SUR_ST_NPARAM];
    int size[SUR_ST_NPARAM];
    int ca, cs;        /* latent action / state channels (4, 16)                            */
    int hq;            /* latent width N/4                                                   */
    int c_mid;         /* channels after the 2nd transposed conv (8)                         */
    float delta;       /* integration step                                                   */
    float mul, add;    /* dscaling(d) = d * mul + add  (Normalize.Inverse with scalar stats) */
    float* partial;    /* [rows][sum(size)]                                                  */
    int rows;
} sur_chunk_params;

/* 0 when the fused kernels implement this geometry (any pointer may be NULL), negative otherwise (sur_last_error()).
 * The fused LayerNorm takes rows of 16, 32, 64, 128, 192 or 256 values: with the reference's strides (2, 2, 1) and the
 * decoder's two transposed convolutions that is N in {64, 128, 256}.  Every launch checks the same and returns -4. */
int sur_geometry_supported(const sur_encoder_params* state_enc, const sur_encoder_params* action_enc, const sur_chunk_params* chunk);

/* Floats per sample of the forward intermediates sur_encoder_forward can save for sur_encoder_backward (0 = this
 * geometry has no saved-activation path).  With `saved` [M, sur_encoder_saved_floats] the backward kernel loads
 * the three blocks' intermediates instead of recomputing them (a third of its time); results are bit-identical. */
int sur_encoder_saved_floats(const sur_encoder_params* p);

/* Optional optimizer step inside the flush launches: torch.optim.Adam(lr, betas, eps) without weight decay /
 * amsgrad (reference: pdecontrol/surrogates/training.py:273-278).  m, v: flat [sum(size)] moment buffers in the
 * pack's parameter order, zero-initialised; step: device counter of completed updates, incremented by the launch;
 * ticket: one zero-initialised unsigned the launch leaves at zero.  With a descriptor the flush writes
 * g = (sum of the partial rows) instead of accumulating into g, and updates the parameters in place. */
typedef struct sur_adam {
    float* m;
    float* v;
    int* step;
    unsigned int* ticket;
    const float* lr;   /* DEVICE scalar: a learning-rate scheduler updates it between replays of a captured step */
    float beta1, beta2, eps;
} sur_adam;

int sur_encoder_forward(void* stream, const sur_encoder_params* p, const float* x, int m, float* z,
                        float* saved /* may be NULL */);
/* dx may be NULL (raw data input).  Accumulates parameter gradients into rows
 * [row_base, row_base + row_count) of p->partial (one row per workgroup; launches that may run
 * concurrently on different streams must be given disjoint row ranges). */
int sur_encoder_backward(void* stream, const sur_encoder_params* p, const float* x, const float* dz, int m,
                         float* dx, int row_base, int row_count, const float* saved /* or NULL = recompute */);
/* Up to three encoder backward jobs (arrays of length njobs; dx is not produced) per launch: all workgroups are
 * dispatched together, so the long action-encoder job does not queue behind the state-encoder jobs.  When every job
 * has a `saved` buffer and a workspace (sur_encoder_workspace_floats(p, m) floats), the backward runs one residual
 * block per launch (three launches, each with a third of the registers and LDS: more workgroups per CU); otherwise one
 * whole-encoder launch. */
int sur_encoder_workspace_floats(const sur_encoder_params* p, int m);
/* One or two encoder forward jobs with `saved` buffers, one residual block per launch (three launches, each carrying
 * all jobs, at most max_workgroups workgroups per job): the large-sample-count form of sur_encoder_forward. */
int sur_encoder_forward_multi(void* stream, int njobs, const sur_encoder_params* const* ps, const float* const* xs, const int* ms,
                              float* const* zs, float* const* saveds, int max_workgroups);
int sur_encoder_backward_multi(void* stream, int njobs, const sur_encoder_params* const* ps, const float* const* xs,
                               const float* const* dzs, const int* ms, const int* row_bases, const int* row_counts,
                               const float* const* saveds, float* const* workspaces /* array may be NULL */);
/* overwrite != 0 (and no Adam descriptor): g = sum of the rows instead of g += sum -- for gradient tensors that start
 * undefined (optimizer.zero_grad(set_to_none=True)), saves the zero-fill.  Every g[i] must be non-NULL, and with an Adam
 * descriptor every w[i] too (the update is applied in place); -1 otherwise, before any launch. */
int sur_flush_encoder_grads(void* stream, const sur_encoder_params* p, const sur_adam* adam /* may be NULL */, int overwrite);

/* Floats per (step, sample) of the forward intermediates sur_chunk_forward saves for sur_chunk_backward (activated
 * gates, c_k, h_k, decoder pre-/post-LayerNorm activations; 14.8 KB at N = 64), or 0 if the latent sizes are not
 * float4-granular (then only the forward is available).  The backward kernels read the intermediates back from HBM
 * instead of recomputing the steps -- HBM capacity and bandwidth are free on this device, dependent-phase latency
 * is not. */
int sur_chunk_saved_floats(const sur_chunk_params* p);

/* Floats of the scratch buffer sur_chunk_backward needs for its split path (0: bad arguments). */
int sur_chunk_workspace_floats(const sur_chunk_params* p, int k, int b);

/* Only the ConvLSTM cell is a recurrence: sur_chunk_forward runs the cell chain with one workgroup per sample, then
 * the decoders of ALL (step, sample) pairs in parallel on every CU, then the integration; sur_chunk_backward (given
 * `saved` and `workspace`) runs the decoder backward of all pairs in parallel, then the cell chain's BPTT.
 *
 * Time-major tensors: xlat_t [K,B,ca,hq]; lstates_t [S,B,cs,hq] (encoded given states, S >= 1);
 * states_t [S,B,1,N] (the given states: bases of the teacher-forced steps); h0, c0 [B,cs,hq] with hc_bstride =
 * cs*hq elements between samples, or ONE [cs,hq] initial state shared by the batch with hc_bstride = 0 (the
 * reference's H0 / C0 parameters, transition.py:254-259).
 * Outputs: h_all, c_all [K,B,cs,hq]; d_all, out_all [K,B,1,N]. */
int sur_chunk_forward(void* stream, const sur_chunk_params* p, const float* xlat_t, const float* lstates_t,
                      const float* states_t, const float* h0, const float* c0, int hc_bstride, int k, int s, int b, float* h_all,
                      float* c_all, float* d_all, float* out_all, float* saved /* NULL: forward only, no backward later */);
/* Upstream gradients (each may be NULL = 0): dd_all / dout_all [K,B,1,N] wrt d_all / out_all;
 * dh_all / dc_all [K,B,cs,hq] wrt h_all / c_all.  Outputs (each may be NULL): dxlat_t [K,B,ca,hq],
 * dlstates_t [S,B,cs,hq], dh0, dc0 [B,cs,hq].  Accumulates parameter gradients into rows
 * [row_base, row_base + row_count) of p->partial (row_count >= B; the parallel decoder backward uses one row
 * per workgroup, up to row_count of them). */
int sur_chunk_backward(void* stream, const sur_chunk_params* p, const float* xlat_t, const float* lstates_t,
                       const float* h0, const float* c0, int hc_bstride, const float* h_all, const float* c_all,
                       const float* dd_all, const float* dout_all, const float* dh_all, const float* dc_all, int k,
                       int s, int b, float* dxlat_t, float* dlstates_t, float* dh0, float* dc0, int row_base, int row_count,
                       const float* saved /* what sur_chunk_forward wrote */, float* workspace /* sur_chunk_workspace_floats */);
/* The backward pass of SEVERAL consecutive TBPTT chunks in the same three launches (TBPTT cuts the graph between
 * chunks, so their cell chains are independent: one workgroup per (chunk, sample); the parallel kernels do not care
 * about chunk borders).  The chunks tile the time axis [0, k_total) of time-major tensors shared by all of them:
 * xlat_t [K,B,ca,hq], h_all / c_all [K,B,cs,hq], saved [K,B,sur_chunk_saved_floats], dd_all [K,B,1,N],
 * dxlat_t [K,B,ca,hq], workspace sur_chunk_workspace_floats(p, k_total, b).  Per chunk: its first `s` steps are
 * teacher forced with lstates_t [s,B,cs,hq] (gradient -> dlstates_t, may be NULL), its initial state is h0 / c0. */
#define SUR_MAX_SPANS 4
typedef struct sur_chunk_span {
    int k0, k1, s;
    const float* lstates_t;
    const float* h0;
    const float* c0;
    int hc_bstride;
    float* dlstates_t;
} sur_chunk_span;
int sur_chunks_backward(void* stream, const sur_chunk_params* p, int nspans, const sur_chunk_span* spans, const float* xlat_t,
                        const float* h_all, const float* c_all, const float* dd_all, int k_total, int b, float* dxlat_t,
                        int row_base, int row_count, const float* saved, float* workspace);
int sur_flush_chunk_grads(void* stream, const sur_chunk_params* p, const sur_adam* adam /* may be NULL */, int overwrite);

/* Latent-space rollout (LatentAutoRegPDESurrogate, the KSLatentConvolutionalLSTM ablation): the same cell and decoder
 * parameters, but the cell output h_k is integrated in LATENT space and the running latent is decoded:
 *   z_{-1} = lstates_t[0],   z_k = z_{k-1} + delta * h_k,   out_k = decoder(z_k)     (p->mul / p->add are not used)
 * Forward: the cell chain as in sur_chunk_forward, an element-wise scan for z, then the decoders of all (step, sample)
 * pairs in parallel on z.  Outputs: h_all, c_all, z_all [K,B,cs,hq]; out_all [K,B,1,N].  With `saved` (same size as for
 * sur_chunk_forward) z_k is stored in the h_k slot of each saved block: the decoder backward takes its input from that
 * slot, the cell backward reads only [gates | c_k] and the cell weight gradients read h_all.
 * Backward: the decoder backward of all pairs on dout_all (may be NULL = 0), a reverse scan that turns the decoder's and
 * the upstream dz_all gradients (dz_all may be NULL) into d loss / d h_k = delta * sum_{j >= k} d loss / d z_j, the cell
 * chain's BPTT and the cell weight gradients.  d loss / d z_{-1} is ADDED to dlstates_t[0] after the cell backward has
 * written the teacher-forcing gradient there.  Other arguments as sur_chunk_backward; the workspace holds
 * sur_latent_workspace_floats(p, k, b) floats: sur_chunk_workspace_floats plus B*cs*hq for d loss / d z_{-1}, which must
 * outlive the cell backward. */
int sur_latent_chunk_forward(void* stream, const sur_chunk_params* p, const float* xlat_t, const float* lstates_t,
                             const float* h0, const float* c0, int hc_bstride, int k, int s, int b, float* h_all, float* c_all,
                             float* z_all, float* out_all, float* saved /* NULL: forward only, no backward later */);
int sur_latent_workspace_floats(const sur_chunk_params* p, int k, int b);
int sur_latent_chunk_backward(void* stream, const sur_chunk_params* p, const float* xlat_t, const float* lstates_t,
                              const float* h0, const float* c0, int hc_bstride, const float* h_all, const float* c_all,
                              const float* dout_all, const float* dz_all, const float* dh_all, const float* dc_all, int k, int s, int b,
                              float* dxlat_t, float* dlstates_t, float* dh0, float* dc0, int row_base, int row_count,
                              const float* saved /* what sur_latent_chunk_forward wrote */,
                              float* workspace /* sur_latent_workspace_floats */);
/* ---- the decoded-mode loss of the latent rollout: csrc/sur_decoded.hip ---------------------------------------------------------
 * Decoded-mode TBPTT loss in one launch (reference: pdecontrol/surrogates/training.py:100-121 with training_mode == "decoded").
 * With prev[b,0] = states[b,0] and prev[b,t] = out_all[t-1,b] (the IC-augmented prediction):
 *   loss          = mean over (b, t < T, i) of (prev[b,t,i] - states[b,t,i])^2       (MSE, reduction "none" + mean)
 *   hsteploss[t]  = the same mean per time step, t < T; hsteploss[0] is exactly 0 (both sides are the same value)
 *   dout_all      = d loss / d out_all  [T,B,1,N]: (float)(2 / (B T N)) * (out_all[t] - states[b,t+1]) for t < T-1, row T-1
 *                   exactly zero; may be NULL
 *   outdeltas[b,t] = ((out_all[t,b] - prev[b,t]) / delta - mean) / stdv              t < T-1: what the chunk loop's
 *                   dscaling.Inverse(diff(cat(states[:, :1], outputs)) / delta) yields across chunk boundaries (a later chunk
 *                   is seeded with the previous chunk's last output)
 *   deltas[b,t]   = ((states[b,t+1] - states[b,t]) / delta - mean) / stdv            t < T-1, the bits sur_tbptt_delta_loss writes
 *   stats         = {mean, unbiased std} of outdeltas, then of deltas (the four "Train ... Delta" metrics)
 * states [B,T,1,N] with element strides as in sur_tbptt_delta_loss; out_all [T,B,1,N] time-major as sur_latent_chunk_forward
 * writes it (row T-1 is not read); outdeltas, deltas [B,T-1,1,N]; hsteploss [T]; loss [1]; stats [4]; partial: scratch of
 * 40*T doubles; ticket: one zero-initialised unsigned the kernel leaves at zero.  Elementwise values are fp32 with one rounding
 * per operation (multiply and add are not contracted); every sum is fp64 and reduced in a fixed order by the workgroup that
 * arrives last; no floating-point atomics.  Refused on the host before any HIP call (-1, the message starts
 * "sur_tbptt_decoded_loss:"): a NULL pointer other than dout_all, B < 1, T < 2, N < 1, B*N > 2^30, a state stride below N,
 * delta == 0, stdv <= 0 (or either NaN).  -2: the launch failed. */
int sur_tbptt_decoded_loss(void* stream, const float* states, long states_bstride, long states_tstride, const float* out_all, int b,
                           int t, int n, float delta, float mean, float stdv, float* outdeltas, float* deltas, float* dout_all,
                           float* hsteploss, float* loss, float* stats, double* partial, unsigned int* ticket);

/* The deltas of a latent rollout in one launch, time-major: d_all[k,b] = ((out_all[k,b] - prev) / delta - mean) / stdv with
 * prev = state0[b] for k = 0 and out_all[k-1,b] afterwards -- dscaling.Inverse(diff(cat(states[:, :1], outputs)) / delta) for a
 * dscaling that is the identity (mean 0, stdv 1) or the inverse of a Normalize with scalar statistics.  state0 [B,1,N] with
 * state_bstride elements between samples; out_all, d_all [K,B,1,N].  Same arithmetic and the same refusals (the message starts
 * "sur_latent_deltas:") as above. */
int sur_latent_deltas(void* stream, const float* state0, long state_bstride, const float* out_all, int k, int b, int n, float delta,
                      float mean, float stdv, float* d_all);

/* The reductions of a surrogate's three parameter packs (two encoders, chunk) in ONE launch; bit j of overwrite_mask
 * is the `overwrite` flag of pack j. */
int sur_flush_all_grads(void* stream, const sur_encoder_params* e0, const sur_adam* a0, const sur_encoder_params* e1,
                        const sur_adam* a1, const sur_chunk_params* c2, const sur_adam* a2, int overwrite_mask);

/* torch.optim.Adam step of up to three packs FROM their gradient tensors g[] in one launch (the optimizer of the eager
 * fused path: reference pdecontrol/surrogates/training.py:273-278 driven by pl.Trainer.fit, mbrl.py:593).  A NULL
 * descriptor skips its pack.  Moments / step counter / device learning rate as in sur_adam above. */
int sur_adam_apply(void* stream, const sur_encoder_params* e0, const sur_adam* a0, const sur_encoder_params* e1,
                   const sur_adam* a1, const sur_chunk_params* c2, const sur_adam* a2);

/* Gradient-norm clipping (pl.Trainer's gradient_clip_val, i.e. torch.nn.utils.clip_grad_norm_ over all parameters) for the
 * step whose Adam update lives on the device: the global norm must be known before the first weight changes, so the
 * clipped step is TWO launches, sur_flush_all_grads_sumsq then sur_clip_adam_apply, with no trip to the host between them.
 *
 * sur_flush_block_count: blocks of sur_flush_all_grads' grid for these three packs (32 columns each, pack by pack) = doubles
 * of `sumsq` below; <= 0: bad argument. */
int sur_flush_block_count(const sur_encoder_params* e0, const sur_encoder_params* e1, const sur_chunk_params* c2);

/* sur_flush_all_grads without Adam descriptors, g = sum of the rows (rows re-zeroed; the same bits), and block k also
 * writes sumsq[k] = the fp64 sum of the squares of the totals it stored (columns past the pack's end count as 0).  The
 * square of an fp32 value is exact in fp64; the 32 squares of a block are added pairwise, partners 16, 8, 4, 2, 1 columns
 * apart.  Every pack, partial buffer and g[i] must be non-NULL, and sumsq; -1 otherwise, before any launch. */
int sur_flush_all_grads_sumsq(void* stream, const sur_encoder_params* e0, const sur_encoder_params* e1,
                              const sur_chunk_params* c2, double* sumsq);

typedef struct sur_clip {
    const double* sumsq; int count;   /* what sur_flush_all_grads_sumsq wrote; count = sur_flush_block_count */
    float max_norm;                   /* > 0 and finite, by value */
    float* total_norm;                /* DEVICE [1], may be NULL: receives the norm BEFORE clipping */
} sur_clip;

/* torch.nn.utils.clip_grad_norm_(all three packs, max_norm) followed by sur_adam_apply, in ONE launch.  Every block
 *   1. folds sumsq[0 .. count) in fp64 in this fixed order: thread j of the block's 256 adds sumsq[j], sumsq[j + 256], ...
 *      in ascending order; the 64 threads of each wavefront are added pairwise, partners 32, 16, 8, 4, 2, 1 lanes apart;
 *      the four wavefronts' sums are added in ascending order -- so every block holds the same bits;
 *   2. total = (float)sqrt(sum);   3. coef = max_norm / (total + 1e-6f) in fp32, then coef = coef > 1 ? 1 : coef;
 *   4. stores g = g * coef (one fp32 multiply, always, as torch does);   5. feeds that product to the Adam update.
 * The norm is taken over the three packs together.  A pack whose descriptor is NULL is scaled but not updated (its step
 * counter stays).  Block 0 alone writes total_norm.  Non-finite values go through the arithmetic as written.  No
 * floating-point atomics; each updated pack's step counter advances once and its ticket is left at zero.  Refused with -1
 * before any launch: a NULL pack, partial buffer, clip or clip->sumsq; a count that is not sur_flush_block_count; a
 * max_norm that is not finite and positive; an incomplete descriptor; a NULL g[i], or a NULL w[i] under a descriptor.
 * (The partial buffers are not read: a pack without one cannot have been through sur_flush_all_grads_sumsq.) */
int sur_clip_adam_apply(void* stream, const sur_encoder_params* e0, const sur_adam* a0, const sur_encoder_params* e1,
                        const sur_adam* a1, const sur_chunk_params* c2, const sur_adam* a2, const sur_clip* clip);

/* Delta-mode TBPTT loss in one launch (reference: pdecontrol/surrogates/training.py:100-121):
 *   deltas[b,t]  = ((states[b,t+1] - states[b,t]) / delta - mean) / stdv          t < T-1   (undscaling forward)
 *   loss         = mean over (b, t < T-1, i) of (d_all[t,b,i] - deltas[b,t,i])^2  (MSE, reduction "none" + mean)
 *   hsteploss[t] = the same mean per time step;  stats = {mean, unbiased std} of the predicted deltas
 *                  d_all[:T-1], then of the true deltas (the four "Train ... Delta" metrics)
 *   dd_all       = d loss / d d_all  [T,B,1,N] (last step zero), may be NULL
 * states [B,T,1,N] with element strides (states_bstride, states_tstride) between samples / time steps -- contiguous
 * batch-major (T*N, N) or a view of time-major storage (N, B*N); d_all [T,B,1,N] time-major as written by sur_chunk_forward; deltas [B,T-1,1,N];
 * hsteploss [T-1]; loss [1]; stats [4]; partial: scratch of 40*T doubles; ticket: one zero-initialised
 * unsigned the kernel leaves at zero.  Sums are fp64 and reduced in a fixed order (deterministic). */
int sur_tbptt_delta_loss(void* stream, const float* states, long states_bstride, long states_tstride, const float* d_all, int b,
                         int t, int n, float delta, float mean,
                         float stdv, float* deltas, float* dd_all, float* hsteploss, float* loss, float* stats,
                         double* partial, unsigned int* ticket);

/* The loss section of validation_step in one launch (reference: pdecontrol/surrogates/training.py:132-174), for the rollout
 * of sur_chunk_forward.  With decoded[t] = states[:, 0] for t = 0 and out_all[t-1] otherwise (the IC-augmented prediction):
 *   deltas[b,t]  = ((states[b,t+1] - states[b,t]) / delta - mean) / stdv                     t < T-1, written if non-NULL
 *   scalars[1]   = delta loss:  mean over (b, t < T-1, i) of (d_all[t,b,i] - deltas[b,t,i])^2
 *   scalars[0]   = scaled loss: mean over (b, t, i) of (decoded - states)^2
 *   loss         = unscaled loss: the same mean of (affine(decoded) - affine(states))^2, hsteploss[t] its mean per time
 *                  step (hsteploss[0] is exactly 0); `decoded` [B,T,1,N] receives affine(decoded) if non-NULL
 * affine is the inverse observation scaling, inv_coef [4][N] = (a, b - a, d - c, c) per column applied in four separately
 * rounded fp32 steps (the kernel keeps its multiply and add uncontracted: `decoded` has the bits of the host transform,
 * and both sides of step 0 go through the same map on the same value, hence hsteploss[0] = 0), or NULL for the identity.  states [B,T,1,N] with element strides as in sur_tbptt_delta_loss; out_all,
 * d_all [T,B,1,N] time-major as sur_chunk_forward writes them (row T-1 of either is not read); hsteploss [T]; loss [1];
 * scalars [2]; partial: scratch of 24*T doubles; ticket: one zero-initialised unsigned the kernel leaves at zero.  Squared
 * errors are fp32, their sums fp64, reduced in a fixed order by the workgroup that arrives last (deterministic).  That
 * workgroup also ADDS the batch's sums to the caller's epoch accumulator accum [3 + T] doubles (may be NULL): accum[0..2] +=
 * the unscaled, scaled and delta error sums, accum[3 + t] += the unscaled error sum of step t -- an epoch's metrics are
 * one copy to the host and a division by counts the host knows.  -1: a bad argument; -2: the launch failed. */
int sur_val_loss(void* stream, const float* states, long states_bstride, long states_tstride, const float* out_all,
                 const float* d_all, int b, int t, int n, float delta, float mean, float stdv, const float* inv_coef,
                 float* deltas, float* decoded, float* hsteploss, float* loss, float* scalars, double* accum, double* partial,
                 unsigned int* ticket);

/* The integration pass of sur_chunk_forward on its own (out_k = base_k + delta * (d_k * mul + add), surrogate.py:108-117):
 * sur_chunk_forward skips it when called with out_all = NULL, so a caller that needs the integrated predictions of a chunk
 * only for reporting (the last TBPTT chunk: nothing is rolled out from them) can queue it off its critical path. */
int sur_chunk_integrate(void* stream, const sur_chunk_params* p, const float* states_t, const float* d_all, int k, int s, int b,
                        float* out_all);

/* sur_tbptt_delta_loss_range in two halves: _rows writes the `deltas` / `dd_all` rows [t_begin, t_end) and their partial sums
 * and takes no ticket -- the backward pass can start from dd_all right away --, _finalize (one workgroup, after every row
 * launch of the loss) reduces the partial sums into loss / hsteploss / stats.  A loss may mix _range launches (early
 * chunks) with ONE _rows launch as long as _finalize follows them all. */
int sur_tbptt_delta_loss_rows(void* stream, const float* states, long states_bstride, long states_tstride, const float* d_all,
                              int b, int t, int n, float delta, float mean, float stdv, float* deltas, float* dd_all,
                              float* hsteploss, float* loss, float* stats, double* partial, unsigned int* ticket, int t_begin,
                              int t_end);
int sur_tbptt_delta_loss_finalize(void* stream, int b, int t, int n, float* hsteploss, float* loss, float* stats, double* partial,
                                  unsigned int* ticket);

/* Fold partial-gradient rows [bases[j], bases[j] + counts[j]) of pack j (0: e0, 1: e1, 2: c2) into row dsts[j] of the same
 * buffer (dst += sum, fixed order; dst outside the folded range) and re-zero them.  A backward branch that ends early
 * (an early TBPTT chunk) folds its own rows, so the step's final sur_flush_all_grads reads one row per branch. */
int sur_fold_rows(void* stream, const sur_encoder_params* e0, const sur_encoder_params* e1, const sur_chunk_params* c2,
                  const int* bases, const int* counts, const int* dsts);

/* The same loss over the time steps [t_begin, t_end) of the T rows only: the launches of one loss -- e.g. one per TBPTT
 * chunk, issued as soon as that chunk's predictions exist, on any streams and in any order -- must cover [0, T) exactly
 * once between them; `loss`, `hsteploss` and `stats` are written by whichever launch finishes last (the ticket counts
 * the workgroups of all T rows), `deltas` / `dd_all` rows by the launch that covers them.  Lets the backward pass of an
 * early chunk start while later chunks are still rolling out (training.py:71-121: gradients are cut between chunks). */
int sur_tbptt_delta_loss_range(void* stream, const float* states, long states_bstride, long states_tstride, const float* d_all,
                               int b, int t, int n, float delta, float mean, float stdv, float* deltas, float* dd_all,
                               float* hsteploss, float* loss, float* stats, double* partial, unsigned int* ticket, int t_begin,
                               int t_end);

/* The window gather of the surrogate-update phase: ONE launch assembles the `states` and `actions` of one TBPTT batch from
 * the packed replay, through the controller's replay-to-world connector (reference: pdecontrol/mbrl/mbrl.py:182-185 applied
 * per item by SubSeqDataset.__getitem__, common/dataset.py:75-81).  For window b < B and step t < L the source row is
 * first[b] + t in logical (packed) order, mapped through rowmap[] when rowmap is non-NULL (the slabs of a device-resident
 * replay) and used as is otherwise:
 *   states[b][t][j]  = affine(obs[row][obs_start + j * obs_stride], obs_coef[:, j])                       j < No
 *   actions[b][t][j] = affine(chain(i), act_out_coef[:, j]),  i = act_start + j * act_stride              j < Na
 *   chain(i)         = acc = a[0] * F[0][i];  acc = fmaf(a[k], F[k][i], acc)  for k = 1 ... A-1,  a[k] = affine(action[row][k],
 *                      act_in_coef[:, k]) -- or, with forcing == NULL, chain(i) = action[row][i] (act_in_coef is not read)
 * with No / Na the columns the sensors keep of obs_width / of forcing_width (of act_width without forcing), and
 * affine(v, (a, b - a, d - c, c)) = ((v - a) / (b - a)) * (d - c) + c in four separately rounded fp32 steps; a NULL coefficient
 * table ([4][columns]) is the identity.  Outputs are fp32 with element strides (bstride, tstride) between windows / steps,
 * so one launch fills a contiguous [B, L, 1, N] tensor (L*N, N) or time-major storage (N, B*N).  A logical row outside
 * [0, total), or a mapped row outside [0, rows), writes NaN to that output row of both outputs and reads nothing.  `first`
 * is a DEVICE pointer (int64); the launch is enqueued on `stream` without synchronisation or allocation.  float4 loads and
 * stores are used per output when its sensor has stride 1, start and widths are multiples of four and every base and
 * stride is 16-byte aligned; the scalar path otherwise. */
typedef struct sur_window_source {
    const float* obs;           /* [rows][obs_width]                                                     */
    const float* actions;       /* [rows][act_width]                                                     */
    const long* rowmap;         /* [total] logical -> physical row, or NULL (then rows is not read)      */
    long total;                 /* logical rows                                                          */
    long rows;                  /* physical rows of obs / actions behind a rowmap                        */
    int obs_width, obs_start, obs_stride;
    const float* obs_coef;      /* [4][No] or NULL                                                       */
    int act_width;              /* A                                                                     */
    const float* act_in_coef;   /* [4][A] or NULL                                                        */
    const float* forcing;       /* [A][forcing_width] or NULL                                            */
    int forcing_width;
    int act_start, act_stride;
    const float* act_out_coef;  /* [4][Na] or NULL                                                       */
} sur_window_source;
/* Refused on the host before any HIP call, with a message that starts "sur_gather_windows:":
 *   -1 a NULL src, obs, actions, first, states or actions pointer     -2 B < 1 or L < 1
 *   -3 obs_width outside 1 ... 1024                                    -4 act_width outside 1 ... 16
 *   -5 a sensor stride < 1                                             -6 a sensor start outside its row
 *   -7 states_width / actions_width is not what the sensor yields      -8 forcing_width < 1 (with a forcing)
 *   -9 total < 1, or rows < 1 behind a rowmap                          -10 an output stride smaller than its row
 *   -20 the launch failed */
int sur_gather_windows(void* stream, const sur_window_source* src, const long* first, int b, int l, float* states,
                       int states_width, long states_bstride, long states_tstride, float* actions, int actions_width,
                       long actions_bstride, long actions_tstride);

/* ---- the fully-connected LSTM baselines (KSAutoRegFullyConnectedLSTM, KSLatentLSTM): csrc/sur_fclstm.hip --------------------
 * Whole-rollout kernels of the fixed network Linear 64 -> 32 -> 16, nn.LSTM(4, 16) on the 4 raw actuator values (gate order
 * i, f, g, o, both biases added), Linear 16 -> 32 -> 64.  Parameters travel as ONE flat fp32 vector in the module's
 * named_parameters() order WITHOUT the frozen H0 / C0 (sur_fc_param_count() = 6 672 floats): the caller expands those into
 * h_in / c_in.
 *
 *   form  SUR_FC_AUTOREG  at a given step k < min(S, K): H = enc(states[k]) (C kept), out_k = states[k] + delta (mul dec(h') + add);
 *                         afterwards H is the LSTM's own and out_k = out_{k-1} + delta (mul dec(h') + add).  inlatents (may
 *                         be NULL: then the re-encoding of the predictions is skipped) is enc(states[k]), then the detached
 *                         enc(out_{k-1}).
 *         SUR_FC_LATENT   z_0 = enc(states[0]), z_{k+1} = z_k + delta h'_k, out_k = dec(z_{k+1}); H is replaced at the given
 *                         steps as above; inlatents[k] is enc(states[k]), then z_k (it carries gradient).  deltas is not
 *                         written (may be NULL); mul / add are not read.
 *   act   SUR_FC_SILU_TANH     SiLU in the encoder and the decoder's first layer, Tanh after its last
 *         SUR_FC_ELU_IDENTITY  ELU likewise, no activation after the last layer
 *
 *   sur_fc_forward   ONE launch: a wave per sample walks all K steps, weights staged in LDS once per workgroup.  `saved`
 *                    (sur_fc_saved_floats(B, K) floats, or NULL when no backward follows) receives 256 floats per
 *                    (sample, step).
 *   sur_fc_backward  TWO launches: the reverse walk (gradients of states, actions, c_in; one workspace row of 304 floats
 *                    per (sample, step)), then the weight gradients as sums of outer products in a fixed order (skipped
 *                    when d_params is NULL).  No floating-point atomics: bit-identical from run to run.
 *
 * Layouts (contiguous fp32 DEVICE pointers): states [B][S][64]; actions [B][K][4], already mapped to the K internal steps;
 * h, c [B][16]; outputs, deltas [B][K][64]; inlatents, outlatents [B][K][16].  h_in never reaches an output (the first
 * step is always a given one), so it is not read and d_h_in receives zeros.  A NULL c_in is zero; a NULL gradient input is
 * zero; a NULL gradient output is not written.  Everything is enqueued on `stream`: no host synchronisation, no device
 * allocation; every argument is checked on the host before the first HIP call.  -1: a bad argument, -2: the launch
 * failed, -4: a layout the kernels do not implement; the reason is in sur_last_error(). */
enum { SUR_FC_AUTOREG = 0, SUR_FC_LATENT = 1 };
enum { SUR_FC_SILU_TANH = 0, SUR_FC_ELU_IDENTITY = 1 };

int sur_fc_param_count(void);

/* 0 when the kernels implement this layout (pure host function) */
int sur_fc_supported(int n, int enc_mid, int latent, int dec_mid, int actions, int form, int act, int nparams);

/* floats of `saved` (256 B K) and of `work` (304 B K); 0 for a non-positive B or K */
long sur_fc_saved_floats(int B, int K);
long sur_fc_workspace_floats(int B, int K);

int sur_fc_forward(void* stream, const float* params, int form, int act, int B, int S, int K, const float* states,
                   const float* actions, const float* h_in, const float* c_in, float delta, float mul, float add,
                   float* outputs, float* deltas, float* inlatents, float* outlatents, float* h_out, float* c_out,
                   float* saved);

int sur_fc_backward(void* stream, const float* params, int form, int act, int B, int S, int K, const float* states,
                    const float* actions, const float* c_in, const float* saved, float delta, float mul,
                    const float* d_outputs, const float* d_deltas, const float* d_inlatents, const float* d_outlatents,
                    const float* d_h_out, const float* d_c_out, float* d_states, float* d_actions, float* d_h_in,
                    float* d_c_in, float* d_params, float* work);

const char* sur_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
