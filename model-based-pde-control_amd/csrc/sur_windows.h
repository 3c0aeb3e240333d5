// sur_windows.h -- what sur_kernels.hip (the C entry and its host validation) hands to sur_windows.hip (the kernel and
// its launcher, built without contraction): the validated arguments of one sur_gather_windows launch.
#ifndef SUR_WINDOWS_H
#define SUR_WINDOWS_H

struct SurWindowsArgs {
    const float* obs;            // [rows][obs_width]
    const float* actions;        // [rows][A]
    const long* rowmap;          // [total] logical -> physical row, or NULL
    const long* first;           // [B] first logical row of each window
    long total, rows;            // logical rows; physical rows of obs / actions
    const float* obs_coef;       // [4][No] or NULL
    const float* act_in_coef;    // [4][A] or NULL
    const float* forcing;        // [A][Lf] or NULL
    const float* act_out_coef;   // [4][Na] or NULL
    float* states;
    float* actions_out;
    long s_bstride, s_tstride, a_bstride, a_tstride;
    int B, L;
    int obs_width, obs_start, obs_stride, No;
    int A, Lf, act_start, act_stride, Na;
    int vec_obs, vec_act;
};

// enqueues the launch on `stream`; returns the hipError_t of the launch as an int (0: hipSuccess)
int sur_windows_launch(void* stream, const SurWindowsArgs& k);

#endif
