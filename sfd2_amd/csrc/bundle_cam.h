// libsfd2hip: what bundle_cam_kernels.hip and api_bundle.hip share -- the device arrays and launchers that sfd2_bundle_adjust_cameras
// adds to those of bundle.h when camera intrinsics are among the unknowns.  fp64 throughout.
#pragma once
#include "bundle.h"

#define SFD2_BA_CAM_K 8               // parameter slots per camera in every per-camera array; slots beyond a camera's own K stay zero
#define SFD2_BA_CAM_WG 256            // threads of a camera's workgroup
// what an active parameter is (BaCamPtrs::slots): the derivative the linearisation takes and the PoseCam word the update moves
#define SFD2_BA_SLOT_NONE -1
#define SFD2_BA_SLOT_F 0              // one focal length: moves f[0] and f[1]
#define SFD2_BA_SLOT_FX 1
#define SFD2_BA_SLOT_FY 2
#define SFD2_BA_SLOT_CX 3
#define SFD2_BA_SLOT_CY 4
#define SFD2_BA_SLOT_K1 5
#define SFD2_BA_SLOT_K2 6
#define SFD2_BA_SLOT_P1 7
#define SFD2_BA_SLOT_P2 8

// The reduced system's vectors (b, x, r, zz, p, q of BaPtrs) are 6 nv + SFD2_BA_CAM_K nc long here: the views' entries, then the cameras'.
// An observation's record keeps its SFD2_BA_REC doubles in BaPtrs::rec, where the kernels of bundle_kernels.hip read them at their own
// stride; its camera block Jk[2][kmax] lies beside it in reck.
struct BaCamPtrs {
    BaPtrs P;
    const int32_t *view_cam;          // [nv]
    const int32_t *slots;             // [nc][SFD2_BA_CAM_K]: SFD2_BA_SLOT_*
    const int64_t *cam_off;           // [nc + 1]: the by-camera list,
    const int32_t *cam_views;         //   views ascending inside a camera
    PoseCam *cams, *cams_trial;       // [nc]
    int32_t *bad;                     // one word: the trial cameras left the finite numbers or the positive focal lengths
    double *reck;                     // [no][2][kmax]
    double *W, *Cp, *gkp, *qkp;       // per view: 6 x 8, 36 (upper triangle of the 8 x 8), 8, 8
    double *C, *gk, *Cinv, *Dk;       // per camera: 64, 8, 64, 8
    int nc, kmax;
};

void launch_bac_linearise(hipStream_t st, const BaCamPtrs &Q, int gate, bool full, bool trial, int loss, double c2);
void launch_bac_cam_build(hipStream_t st, const BaCamPtrs &Q, int gate);
void launch_bac_cam_precond(hipStream_t st, const BaCamPtrs &Q);
void launch_bac_point_apply(hipStream_t st, const BaCamPtrs &Q, int gate, const double *x);
void launch_bac_apply(hipStream_t st, const BaCamPtrs &Q, int gate, bool rhs);
void launch_bac_pcg_init(hipStream_t st, const BaCamPtrs &Q);
void launch_bac_pcg_step(hipStream_t st, const BaCamPtrs &Q, double tol2, int max_iters);
void launch_bac_update_cams(hipStream_t st, const BaCamPtrs &Q);
void launch_bac_veto(hipStream_t st, const BaCamPtrs &Q);
void launch_bac_commit_cams(hipStream_t st, const BaCamPtrs &Q);
