// Covisibility clustering of retrieved frames (it_loc/localize_cv2.py:87-117 do_covisibility_clustering) on gfx950.
//
// One 256-thread workgroup per query, grid-striding over the queries.  A query is a list of k <= 256 distinct images.  There is an
// edge i -> j between two list positions when image j occurs in the track of a point that image i observes; a frame of the list that
// is not yet visited opens a cluster that takes every not-yet-visited frame reachable from it over those edges, in list order.
//
//   slots      image -> list position, 16 bits per image (256 positions plus "none" do not fit a byte).  In LDS when n_images fits
//              (SFD2_CLUSTER_LDS_IMAGES), else a row of global scratch per workgroup.  Filled with "none" once; a query sets its k
//              entries and un-sets exactly those when it is done, so the cost per query does not grow with the map.
//   adjacency  k x k bits in LDS (256 rows of 8 words).  One wave per frame, its lanes stride over the frame's observations and walk
//              each point's track; a track element whose image has a slot sets one bit (LDS atomic OR, skipped when already set).
//   closure    per seed in list order: the reach set grows by the rows of its new members, masked by the visited set, until a round
//              adds nothing -- a fixed point, not a fixed number of rounds (a chain through all 256 frames needs 255).
//   ranks      cluster sizes by popcount; rank = number of clusters that are larger, or equally large and created earlier.
// Integer and bit operations only: a query's output depends on the query and the map alone.
#include "sfd2_internal.h"
#include <algorithm>

namespace {

#define CLU_MAX 256                 // SFD2_CLUSTER_MAX_FRAMES
#define CLU_WORDS (CLU_MAX / 32)
#define CLU_NONE 0xffffu

template <bool GLOBAL>
__global__ __launch_bounds__(256) void covis_cluster_kernel(const int64_t *__restrict__ obs_off, const int32_t *__restrict__ obs_point, int n_images,
                                                            const int64_t *__restrict__ trk_off, const int32_t *__restrict__ trk_img,
                                                            const int64_t *__restrict__ frame_off, const int32_t *__restrict__ frames, int nq,
                                                            uint16_t *scratch, int32_t *__restrict__ cluster, int32_t *__restrict__ n_clusters)
{
    extern __shared__ __align__(16) unsigned char cluster_smem[];
    __shared__ unsigned adj[CLU_MAX * CLU_WORDS];
    __shared__ unsigned reach[CLU_WORDS], nxt[CLU_WORDS], visited[CLU_WORDS];
    __shared__ int fr[CLU_MAX], cid[CLU_MAX], csize[CLU_MAX], crank[CLU_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint16_t *slot = GLOBAL ? scratch + (size_t)blockIdx.x * n_images : reinterpret_cast<uint16_t *>(cluster_smem);
    if (!GLOBAL) {                                                 // the global rows arrive filled with "none"
        for (int j = tid; j < n_images; j += 256) slot[j] = CLU_NONE;
    }
    __syncthreads();
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t f0 = frame_off[q];
        const int k = (int)(frame_off[q + 1] - f0);                // 0 .. CLU_MAX, checked by the caller
        if (k == 0) {
            if (tid == 0) n_clusters[q] = 0;
            continue;
        }
        for (int j = tid; j < CLU_MAX * CLU_WORDS; j += 256) adj[j] = 0;
        if (tid < CLU_WORDS) visited[tid] = 0;
        if (tid < k) {
            const int f = frames[f0 + tid];
            fr[tid] = f;
            slot[f] = (uint16_t)tid;
        }
        __syncthreads();
        // adjacency: wave w takes positions w, w + 4, ...
        for (int i = wave; i < k; i += 4) {
            const int f = fr[i];
            for (int64_t o = obs_off[f] + lane; o < obs_off[f + 1]; o += 64) {
                const int p = obs_point[o];
                for (int64_t t = trk_off[p]; t < trk_off[p + 1]; ++t) {
                    const unsigned j = slot[trk_img[t]];
                    if (j == CLU_NONE) continue;
                    unsigned *w = adj + i * CLU_WORDS + (j >> 5);
                    const unsigned bit = 1u << (j & 31);
                    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) atomicOr(w, bit);
                }
            }
        }
        __syncthreads();
        // closure, seed by seed in list order; every thread follows the same control flow (it reads the sets from LDS)
        int created = 0;
        for (int s = 0; s < k; ++s) {
            if ((visited[s >> 5] >> (s & 31)) & 1) continue;   // uniform: written before the barrier that ended the last seed
            if (tid < CLU_WORDS) reach[tid] = nxt[tid] = (tid == (s >> 5)) ? 1u << (s & 31) : 0u;
            bool expanded = false;
            __syncthreads();
            for (;;) {
                const bool in = tid < k && ((reach[tid >> 5] >> (tid & 31)) & 1);
                if (in && !expanded) {                             // a member adds its row once
                    expanded = true;
#pragma unroll
                    for (int w = 0; w < CLU_WORDS; ++w) {
                        const unsigned v = adj[tid * CLU_WORDS + w] & ~visited[w] & ~reach[w];
                        if (v) atomicOr(nxt + w, v);
                    }
                }
                __syncthreads();
                bool changed = false;
#pragma unroll
                for (int w = 0; w < CLU_WORDS; ++w) changed |= nxt[w] != reach[w];
                __syncthreads();                                   // compared everywhere before reach moves
                if (!changed) break;
                if (tid < CLU_WORDS) reach[tid] = nxt[tid];
                __syncthreads();
            }
            if (tid < k && ((reach[tid >> 5] >> (tid & 31)) & 1)) cid[tid] = created;
            if (tid == 0) {
                int n = 0;
#pragma unroll
                for (int w = 0; w < CLU_WORDS; ++w) n += __popc(reach[w]);
                csize[created] = n;
            }
            if (tid < CLU_WORDS) visited[tid] |= reach[tid];
            ++created;
            __syncthreads();
        }
        __syncthreads();
        // ranks: larger first, equal sizes in creation order
        if (tid < created) {
            const int mine = csize[tid];
            int r = 0;
            for (int b = 0; b < created; ++b) {
                const int other = csize[b];
                r += (other > mine || (other == mine && b < tid)) ? 1 : 0;
            }
            crank[tid] = r;
        }
        __syncthreads();
        if (tid < k) {
            cluster[f0 + tid] = crank[cid[tid]];
            slot[fr[tid]] = CLU_NONE;                              // only what this query set
        }
        if (tid == 0) n_clusters[q] = created;
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_covis_clusters(hipStream_t st, const int64_t *obs_off, const int32_t *obs_point, int n_images, const int64_t *trk_off,
                                 const int32_t *trk_img, const int64_t *frame_off, const int32_t *frames, int nq, int global_slots, int blocks,
                                 uint16_t *scratch, int32_t *cluster, int32_t *n_clusters)
{
    if (global_slots) {
        covis_cluster_kernel<true><<<dim3(blocks), dim3(256), 0, st>>>(obs_off, obs_point, n_images, trk_off, trk_img, frame_off, frames, nq, scratch,
                                                                      cluster, n_clusters);
    } else {
        const size_t lds = ((size_t)n_images * 2 + 15) & ~(size_t)15;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(covis_cluster_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        covis_cluster_kernel<false><<<dim3(blocks), dim3(256), lds, st>>>(obs_off, obs_point, n_images, trk_off, trk_img, frame_off, frames, nq, nullptr,
                                                                         cluster, n_clusters);
    }
    return hipGetLastError();
}
