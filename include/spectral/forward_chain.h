/*
 * spectral/forward_chain.h -- the free-running chain entry point of libspectral_hip.so (kernel: csrc/fno.hip; binding:
 * pdecontrol/surrogates/fno_hip.py, CHAIN_SYMBOLS).  An extension of ../spectral_hip.h, whose fno_weights, geometry
 * rules and fno_last_error() it uses unchanged.
 *
 *   fno_forward_chain    all free-running steps of a rollout in one launch.  One workgroup per sample b (the thread count
 *                  and the LDS layout of fno_forward's inference kernel) copies the twiddle matrix into LDS once and then
 *                  evaluates the network `steps` times, each step starting from the row the step before produced:
 *                      delta[k][b] = model(base_k, act[k][b]),  out[k][b] = base_k + cscale * delta[k][b] + cshift,
 *                      base_0 = u0[b],  base_k = out[k - 1][b].
 *                  delta[k][b] and out[k][b] equal, byte for byte, what `steps` successive launches
 *                      fno_forward(w, ..., nb, pairs = nb, u = (k == 0 ? u0 : out[k - 1]), ..., act + k * a_stride_t, ...,
 *                                  cscale, cshift, delta[k], out[k], NULL, NULL, 0, 0)
 *                  write: the same arithmetic on the same device functions.  The base row travels from step to step in LDS
 *                  (a workgroup never reads `out` back), so the launch needs no fence and no atomics.  Inference only:
 *                  no pre-activation and no spectrum is stored.
 *
 * It is declared here and not in spectral_hip.h because that header's list of functions is pinned, name by name;
 * tests/test_fno_chain_host.py holds this header, its binding table and the library to each other.
 *
 * The struct and the fno_weights it points to are HOST structs read during the call; every pointer inside them is a DEVICE
 * pointer and travels to the kernel by value.  Strides are in floats.  The launch is asynchronous on the given
 * hipStream_t, synchronises nothing and allocates no device memory; as for fno_forward, the first use of a width N on a
 * device builds the twiddle matrix and is refused inside a stream capture: run one eager call first.
 */
#ifndef SPECTRAL_FORWARD_CHAIN_H
#define SPECTRAL_FORWARD_CHAIN_H

#include "../spectral_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fno_chain_args {
    const fno_weights* w;            /* HOST struct of device pointers, by value into the launch */
    float cscale, cshift;
    const float* u0; long u0_stride_b;                 /* [nb][n]: the state step 0 starts from */
    const float* act; long a_stride_t, a_stride_b;     /* [steps][nb][n] action field */
    float* delta;                    /* [steps][nb][n] contiguous, time major */
    float* out;                      /* [steps][nb][n] contiguous, time major */
    int steps;                       /* >= 1 */
} fno_chain_args;

/* Refusals, all decided on the host before any HIP call: -1 a NULL a, u0, act, delta or out, an incomplete fno_weights,
 * steps < 1, nb < 1, a stride that is walked (u0_stride_b and a_stride_b with nb > 1, a_stride_t with steps > 1) smaller
 * than a row of n floats, out or delta overlapping u0, act or each other (u0 may END where out begins: the row just before
 * it in one buffer); -4 a geometry other than width 32, 16 modes, 4 layers, n a power of two in [64, 512].
 * -2: a HIP call failed; -4 also for the first use of a width inside a stream capture. */
int fno_forward_chain(void* stream, int width, int modes, int layers, int n, int nb, const fno_chain_args* a);

#ifdef __cplusplus
}
#endif

#endif
