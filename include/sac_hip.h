/*
 * sac_hip.h -- C ABI of libsac_hip.so: gfx950 kernels of the soft actor-critic agent (pdecontrol/sac/sac.py: SAC.act,
 * SAC.update; kernels: csrc/sac.hip).
 *
 * The networks are the reference's (pdecontrol/sac/policies.py): GaussianPolicy obs -> 256 -> 256 -> (mean, log_std) and
 * QNetwork, two heads (obs | action) -> 256 -> 256 -> 1, hidden = 256, obs_dim in {64, 128, 256}, act_dim 1 ... 16, any
 * batch size B >= 1.  Parameters stay the module's own tensors: `sac_state` carries one device pointer per tensor in
 * named_parameters() order (policy: linear1, linear2, mean_linear, log_std_linear; critic and target: linear1 ... linear6;
 * weight before bias), with the torch.optim.Adam moments exp_avg (`*_m`) and exp_avg_sq (`*_v`) in the same order.
 *
 *   sac_policy_forward   ONE launch: a workgroup per 16 samples runs the policy with its activations in LDS.
 *   sac_update           one reference update (sac.py:75-132) as FIVE launches, one chain on `stream`:
 *                          1 critic pass    per 16-sample tile: policy and target critic on nxtobs -> target value, critic
 *                                           forward on (obs, actions), MSE, critic backward down to the layer gradients
 *                          2 critic wgrad   every workgroup owns tiles of dW (bias = one more column), reduces over all
 *                                           samples in order, applies Adam and (every target_update_interval) the Polyak
 *                                           average of the target to its tile
 *                          3 policy pass    per tile: policy on obs, the UPDATED critic on (obs, pi), min, backward through
 *                                           the critic's action columns and the tanh-Gaussian head into the policy layers
 *                          4 policy wgrad   as 2, Adam only
 *                          5 finalize       one workgroup: statistics, log_alpha's Adam step (alpha for the NEXT update),
 *                                           step counts and the update counter
 *   sac_grads            the same five launches with every state write suppressed: launches 2, 4 and 5 store the gradients
 *                        to the caller's buffers instead (so the policy gradient is against the not-updated critic).
 *
 * No float atomics: every reduction over the batch is an ordered sum, results are bit-identical run to run.  The step
 * counts and the update counter live in `counters` (device int32[8]: critic step, policy step, log_alpha step, updates,
 * terminated samples seen so far) and are advanced by launch 5, so a captured graph replays correctly.
 *
 * Layouts (contiguous fp32, DEVICE pointers unless stated): obs, nxtobs [B][obs_dim]; actions, noise [B][act_dim];
 * rewards, terminated [B]; stats [8]: critic loss, policy loss, alpha loss, alpha, mean reward, terminated samples of this
 * batch.  `sac_config` and `sac_state` themselves are HOST structs, read during the call.  Everything is enqueued on
 * `stream`: no host synchronisation, no device allocation.  Return 0 on success, negative on error (sac_last_error()).
 */
#ifndef SAC_HIP_H
#define SAC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SAC_POLICY_TENSORS 8
#define SAC_CRITIC_TENSORS 12

typedef struct sac_config {
    int obs_dim, act_dim, hidden;
    int auto_alpha;              /* automatic entropy tuning: log_alpha takes its Adam step in launch 5 */
    int target_update_interval;
    float gamma, tau, target_entropy;
    float lr[3], beta1[3], beta2[3], eps[3];   /* Adam of critic, policy, log_alpha */
} sac_config;

typedef struct sac_state {
    float* policy[SAC_POLICY_TENSORS];
    float* policy_m[SAC_POLICY_TENSORS];
    float* policy_v[SAC_POLICY_TENSORS];
    float* critic[SAC_CRITIC_TENSORS];
    float* critic_m[SAC_CRITIC_TENSORS];
    float* critic_v[SAC_CRITIC_TENSORS];
    float* target[SAC_CRITIC_TENSORS];
    float* log_alpha;            /* [1]; with its moments NULL unless auto_alpha */
    float* log_alpha_m;
    float* log_alpha_v;
    float* alpha;                /* [1]: the entropy coefficient this update uses; launch 5 writes exp(log_alpha) */
    int* counters;               /* int32[8], see above */
    const float* act_scale;      /* [act_dim] */
    const float* act_bias;       /* [act_dim] */
} sac_state;

/* 0 when the kernels implement this geometry, else a negative code with the reason in sac_last_error() */
int sac_supported(int obs_dim, int act_dim, int hidden);

/* floats of the `work` buffer sac_update / sac_grads need for batch B (negative: unsupported geometry) */
long sac_workspace_floats(int obs_dim, int act_dim, int hidden, int B);

/* action = tanh(mean + exp(log_std) * noise) * scale + bias (noise NULL: zero); logp [B] and mean_action [B][act_dim]
 * (= tanh(mean) * scale + bias) are optional.  Only st->policy, act_scale and act_bias are read. */
int sac_policy_forward(void* stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* noise,
                       float* action, float* logp, float* mean_action);

int sac_update(void* stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* actions,
               const float* nxtobs, const float* rewards, const float* terminated, const float* noise_next,
               const float* noise_cur, float* stats, float* work);

/* g_critic [12], g_policy [8]: HOST arrays of device pointers shaped like the parameters; g_log_alpha [1] or NULL */
int sac_grads(void* stream, const sac_config* cfg, const sac_state* st, int B, const float* obs, const float* actions,
              const float* nxtobs, const float* rewards, const float* terminated, const float* noise_next,
              const float* noise_cur, float* stats, float* work, float* const* g_critic, float* const* g_policy,
              float* g_log_alpha);

const char* sac_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
