// libsfd2hip: sfd2_homography_batch -- one launch of homography_kernels.hip through api_fundamental.hip's checking, packing and scratch
// layer (pairs_batch): the problem and the result have sfd2_fundamental_batch's layout, the matrix is H.
#include <cstddef>
#include "sfd2_ctx.h"

static_assert(sizeof(sfd2_homography_problem) == sizeof(sfd2_fundamental_problem) && offsetof(sfd2_homography_problem, n) == offsetof(sfd2_fundamental_problem, n) &&
                  offsetof(sfd2_homography_problem, points2D_0) == offsetof(sfd2_fundamental_problem, points2D_0) &&
                  offsetof(sfd2_homography_problem, points2D_1) == offsetof(sfd2_fundamental_problem, points2D_1) &&
                  offsetof(sfd2_homography_problem, max_error_px) == offsetof(sfd2_fundamental_problem, max_error_px),
              "sfd2_homography_problem has sfd2_fundamental_problem's layout");
static_assert(sizeof(sfd2_homography_result) == sizeof(sfd2_fundamental_result) && offsetof(sfd2_homography_result, success) == offsetof(sfd2_fundamental_result, success) &&
                  offsetof(sfd2_homography_result, num_inliers) == offsetof(sfd2_fundamental_result, num_inliers) &&
                  offsetof(sfd2_homography_result, num_trials) == offsetof(sfd2_fundamental_result, num_trials) &&
                  offsetof(sfd2_homography_result, H) == offsetof(sfd2_fundamental_result, F),
              "sfd2_homography_result has sfd2_fundamental_result's layout");

extern "C" int sfd2_homography_batch(sfd2_ctx *c, const sfd2_homography_problem *problems, int k, const sfd2_two_view_conf *conf,
                                     sfd2_homography_result *results, uint8_t *inlier_mask_u8, int flags)
{
    return pairs_batch("sfd2_homography_batch", 4, launch_homography, c, reinterpret_cast<const sfd2_fundamental_problem *>(problems), k, conf,
                       reinterpret_cast<sfd2_fundamental_result *>(results), inlier_mask_u8, flags);
}
