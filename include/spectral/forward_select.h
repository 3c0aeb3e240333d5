/*
 * spectral/forward_select.h -- the member-select entry point of libspectral_hip.so (kernel: csrc/fno.hip; binding:
 * pdecontrol/surrogates/fno_hip.py, SELECT_SYMBOLS).  An extension of ../spectral_hip.h, whose fno_weights, geometry
 * rules and fno_last_error() it uses unchanged.
 *
 *   fno_forward_select   one imagined step of an ensemble of FNO surrogates.  The FNO surrogate is stateless, so env b at
 *                  step t needs the evaluation of member chosen[t][b] alone: one workgroup per env (the thread count and
 *                  the LDS layout of fno_forward's inference kernel) reads its member index, takes that member's weight
 *                  pointers out of the kernel arguments and evaluates the network once,
 *                      out[b] = u[b] + cscale[pick] * model_pick(u[b], act[b]) + cshift[pick].
 *                  Row b equals, byte for byte, row b of `out` of
 *                      fno_forward(&w[pick], ..., nb, pairs = nb, u, 0, n, act, 0, n, cscale[pick], cshift[pick], delta, out,
 *                                  NULL, NULL, 0, 0):
 *                  the same arithmetic reading other pointers.  No delta, pre-activation or spectrum is stored.
 *                  t = step ? step[0] : 0; for t outside [0, T) every workgroup leaves and nothing is written.  A member
 *                  index outside [0, members) reads no weight and leaves row b all NaN (ro_settle's poison convention).
 *                  step[0] is only READ, which keeps the counter rule of rollout_hip.h: ro_act_chain publishes step[0],
 *                  ro_settle reads it and publishes step[1]; this launch sits between the two.
 *
 * It is declared here and not in spectral_hip.h because that header's list of functions is pinned, name by name;
 * tests/test_fno_select_host.py holds this header, its binding table and the library to each other.
 *
 * The structs are HOST structs read during the call; the weights, scales and shifts of the first `members` members travel
 * to the kernel by value.  As for fno_forward, the first use of a width N on a device builds the twiddle matrix and is
 * refused inside a stream capture: run one eager call first.
 */
#ifndef SPECTRAL_FORWARD_SELECT_H
#define SPECTRAL_FORWARD_SELECT_H

#include "../spectral_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FNO_MAX_MEMBERS 8            /* = RO_MAX_MEMBERS */

typedef struct fno_select_args {
    const fno_weights* w;            /* HOST array [members] of device-pointer structs, read during the call */
    const float* cscale;             /* HOST [members]: delta * dscaling scale, per member */
    const float* cshift;             /* HOST [members] */
    int members;                     /* 1 ... FNO_MAX_MEMBERS */
    const int* chosen;               /* DEVICE [T][nb] member per env and step; NULL with one member */
    const int* step;                 /* DEVICE int32[2] of rollout_hip.h; step[0] is READ, nothing is written; NULL: slot 0 */
    int T;                           /* slots of `chosen` */
    const float* u;                  /* DEVICE [nb][n] world state */
    const float* act;                /* DEVICE [nb][n] action field (the world's action row; its width must be n) */
    float* out;                      /* DEVICE [nb][n]; must not alias u */
} fno_select_args;

/* Refusals, all decided on the host before any HIP call: -1 a NULL a, w, cscale, cshift, u, act or out, an incomplete
 * fno_weights among the first `members`, members outside 1 ... FNO_MAX_MEMBERS, members > 1 without `chosen`, T < 1,
 * out == u, nb < 1; -4 a geometry other than width 32, 16 modes, 4 layers, n a power of two in [64, 512].
 * -2: a HIP call failed; -4 also for the first use of a width inside a stream capture. */
int fno_forward_select(void* stream, int width, int modes, int layers, int n, int nb, const fno_select_args* a);

#ifdef __cplusplus
}
#endif

#endif
