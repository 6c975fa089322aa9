// libsfd2hip: what mapper_kernels.hip and api_mapper.hip share -- the launchers of the incremental mapper's bookkeeping passes
// (DESIGN.md section 15).  Integer work except the filter, which is fp64; every launcher queues on the given stream and returns.
#pragma once
#include "sfd2_internal.h"

#define SFD2_MAP_LONG_TRACK 64        // a track (or point) with more observations than this gets a wave of its own, else one lane
#define SFD2_MAP_WG 256               // threads of the flat kernels' blocks and of a candidate's workgroup

// restrict: keep[t] = the track has registered observations in two distinct views, cnt[t] = its registered observations (0 when not kept)
void launch_mapper_restrict_count(hipStream_t st, const int32_t *short_ids, int n_short, const int32_t *long_ids, int n_long, const int64_t *off,
                                  const int32_t *obs_view, const unsigned char *reg, int32_t *keep, int32_t *cnt);
// tpos / opos: the exclusive scans of keep / cnt; totals[2] = (T', O'); sub_off gets T' + 1 entries
void launch_mapper_restrict_scatter(hipStream_t st, const int32_t *short_ids, int n_short, const int32_t *long_ids, int n_long, int n_tracks,
                                    const int64_t *off, const int32_t *obs_view, const float2 *obs_xy, const unsigned char *reg, const int32_t *keep,
                                    const int32_t *cnt, const int32_t *tpos, const int32_t *opos, int32_t *sub_track, int64_t *sub_off, int32_t *sub_obs,
                                    int32_t *sub_view, float2 *sub_xy, int64_t *totals);
// filter, per observation: reprojection error, keep flag, the ray from the point to the view's centre
void launch_mapper_filter_obs(hipStream_t st, const TriViewDev *views, const double *xyz, const int32_t *obs_view, const int32_t *obs_pt,
                              const double2 *obs_xy, int64_t n, double max_err, double *err, unsigned char *keep, double *ray);
// filter, per point: live flag, mean kept error, largest angle between two kept rays (degrees)
void launch_mapper_filter_points(hipStream_t st, const int32_t *short_ids, int n_short, const int32_t *long_ids, int n_long, const int64_t *off,
                                 const int32_t *obs_view, const double *err, const unsigned char *keep, const double *ray, double min_angle_deg,
                                 unsigned char *live, double *perr, double *pangle);
// tlive[t] += 1 per live point of track t (tlive arrives zeroed); tfirst[t] = the first point of track t (tfirst arrives filled with -1; may be null)
void launch_mapper_track_points(hipStream_t st, const int32_t *point_track, const unsigned char *point_live, int n_points, int32_t *tlive, int32_t *tfirst);
// counts[v] += tlive[track of o] for every observation o of an unregistered view v (counts arrives zeroed)
void launch_mapper_visible(hipStream_t st, const int64_t *off, int n_tracks, const int32_t *obs_view, int64_t n_obs, const unsigned char *reg,
                           const int32_t *tlive, unsigned long long *counts);
// assemble: total[c] = correspondences of candidate c (total[k] is not written)
void launch_mapper_assemble_count(hipStream_t st, const int32_t *cand, int k, const int64_t *view_off, const int32_t *view_obs, const int64_t *off,
                                  int n_tracks, const int32_t *tlive, int64_t *total);
void launch_mapper_assemble_scatter(hipStream_t st, const int32_t *cand, int k, const int64_t *view_off, const int32_t *view_obs, const int64_t *off,
                                    int n_tracks, const float2 *obs_xy, const int32_t *tfirst, const int32_t *point_track,
                                    const unsigned char *point_live, int n_points, const double *xyz, const int64_t *offsets, double2 *p2, double *p3,
                                    int32_t *src_obs, int32_t *src_point);
