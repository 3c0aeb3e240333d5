/*
 * replay/slabs.h -- the slabs of a device-resident replay (pdecontrol/mbrl/device_replay.py): one tensor per field in
 * DeviceSubSeqStore.tensors dtypes, `rows` rows each.  A HOST struct of DEVICE pointers, read during the call.  The one
 * struct every entry that places transitions takes, under the name its header gives it: rp_slab (../replay_hip.h:
 * rp_append), ks_record (../kspde.h: ks_record_device) and bg_slabs (../burgers_hip.h: bg_record).  ctypes mirror:
 * hipbind.Slabs.
 */
#ifndef REPLAY_SLABS_H
#define REPLAY_SLABS_H

typedef struct replay_slabs {
    float* obs;                      /* [rows][N] */
    float* actions;                  /* [rows][A] */
    float* nxtobs;                   /* [rows][N] */
    float* rewards;                  /* [rows] */
    unsigned char* terminated;       /* [rows] */
    unsigned char* truncated;        /* [rows] */
    int* steps;                      /* [rows] */
    long rows;
} replay_slabs;

#endif
