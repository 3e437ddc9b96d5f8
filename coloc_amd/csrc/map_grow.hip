// map_grow.hip -- the map grown past the seed pair on the device (include/coloc_hip.h: clc_map_build_grow_dev,
// clc_map_init_grow_batch_dev, clc_map_update_grow_batch_dev, clc_map_resect_build_dev): the loop `for (auto resectionId :
// resectionList) resectionCamera(resectionId)` of Reconstructor::reconstructScene (reference include/coloc/Reconstructor.hpp:153-154,
// 259-415) and setupMapDatabase over the landmarks it leaves (colocData.hpp:89-121).  The state is per TRACK -- Landmarks is a map keyed by track id --: X[t] and obs[t], one
// bit per camera, 0 = no landmark.  Launches, all enqueue-only on one stream; no kernel holds a lock or waits for another workgroup:
//   grow_clear_kernel / grow_scatter_kernel   one thread per track / per seed map row: obs = 0, then the staged seed map into X / obs
//   resect_gather_kernel   ONE workgroup: the ordered compaction of wg_compact.h over the tracks with a landmark that hold the camera ->
//                          X | x (get_ud_pixel) | track ids | rows in the layout the a-contrario staging launch reads; the count last
//   grow_kernel            one thread per track of the camera: a landmark that exists gains the camera; a track without one is
//                          triangulated against the valid cameras in ascending order (grow_point, map_math.h) until one is accepted;
//                          observation_ok decides the mask.  A thread touches its own track only: no atomics
//   grow_compact_kernel    ONE workgroup: the ordered compaction over the tracks with a landmark -> the map's rows in track-id order,
//                          row = { X, track, camera of the lowest set bit, that camera's row, mask }; the count last
// The solve between the gather and the grow is the a-contrario launch path itself (resect_solve, pose_batch.hip).  Some 10 k tracks:
// latency-bound like the seed launch; nothing here is tuned and nothing is claimed of its speed.  The bundle adjustment that follows the
// loop in the reference (Reconstructor.hpp:160-161) works on this state between the last grow_kernel and grow_compact_kernel: map_ba.hip.
#include "clc_ctx.h"
#include "map_math.h"
#include "ud_pixel.h"
#include "wg_compact.h"

#include <cmath>

namespace clc {

namespace {

constexpr int kOneGroup = 1024;              // the two ordered compactions
constexpr int kWide = 256;                   // the kernels with one thread per track

__device__ __forceinline__ int32_t track_count(const GrowState& s)
{
    const int32_t n = s.n_tracks[0];
    return n < 0 ? 0 : (n > s.cap ? s.cap : n);
}

__device__ __forceinline__ void track_pixel(const GatherSide& side, const int32_t row, const float* scale, double* out)
{
    float fx, fy;
    feature_position(side.kps, side.feat, side.feat_stride, (uint32_t)row, scale, &fx, &fy);
    ud_pixel(fx, fy, side.cam, out);
}

struct Scales { float v[CLC_MAX_LEVELS]; };

__global__ __launch_bounds__(kWide) void grow_clear_kernel(const GrowState s)
{
    const int32_t t = (int32_t)(blockIdx.x * kWide + threadIdx.x);
    if (t < s.cap) s.obs[t] = 0u;
}

__global__ __launch_bounds__(kWide) void grow_scatter_kernel(const GrowState s, const int32_t* __restrict__ map_track, const double* __restrict__ map_X,
                                                            const int32_t n_rows, const uint32_t seed_bits)
{
    const int32_t i = (int32_t)(blockIdx.x * kWide + threadIdx.x);
    if (i >= n_rows) return;
    const int32_t t = map_track[i];
    if (t < 0 || t >= s.cap) return;
    s.X[3 * (size_t)t] = map_X[3 * (size_t)i]; s.X[3 * (size_t)t + 1] = map_X[3 * (size_t)i + 1]; s.X[3 * (size_t)t + 2] = map_X[3 * (size_t)i + 2];
    s.obs[t] = seed_bits;
}

__global__ __launch_bounds__(kOneGroup) void resect_gather_kernel(const GrowState s, const GatherSide side, const Scales scale, const int32_t camera,
                                                                  const ResectOut o)
{
    __shared__ uint32_t s_wave[kOneGroup / 64];
    const int32_t nt = track_count(s);
    uint32_t base = 0;
    for (int32_t t0 = 0; t0 < nt; t0 += kOneGroup) {
        const int32_t t = t0 + (int32_t)threadIdx.x;
        const int32_t r = t < nt ? s.table[(size_t)t * s.n_cams + camera] : -1;
        const bool ok = r >= 0 && s.obs[t] != 0u;
        uint32_t total;
        const uint32_t i = base + ordered_slot<kOneGroup>(ok, s_wave, &total);
        if (ok && i < (uint32_t)o.cap) {
            const double* X = s.X + 3 * (size_t)t;
            o.X[3 * (size_t)i] = X[0]; o.X[3 * (size_t)i + 1] = X[1]; o.X[3 * (size_t)i + 2] = X[2];
            track_pixel(side, r, scale.v, o.x + 2 * (size_t)i);
            if (o.track) o.track[i] = t;
            if (o.row) o.row[i] = r;
            if (o.h_track) o.h_track[i] = t;
            if (o.h_row) o.h_row[i] = r;
        }
        base += total;
    }
    // the count comes out last: the lists and the mirrors are complete and visible system-wide before the word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        if (o.d_n) *o.d_n = (int32_t)base;
        if (o.h_n) __hip_atomic_store(o.h_n, base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(kWide) void grow_kernel(const GrowState s, const GrowCams cams, const int32_t I)
{
    const int32_t t = (int32_t)(blockIdx.x * kWide + threadIdx.x);
    if (t >= track_count(s)) return;
    const int32_t* row = s.table + (size_t)t * s.n_cams;
    const int32_t ri = row[I];
    if (ri < 0) return;
    uint32_t obs = s.obs[t], cand = 0u;
    double X[3];
    if (obs != 0u) {
        cand = 1u << I;
        X[0] = s.X[3 * (size_t)t]; X[1] = s.X[3 * (size_t)t + 1]; X[2] = s.X[3 * (size_t)t + 2];
    } else {
        double xi[2];
        track_pixel(cams.side[I], ri, cams.scale, xi);
        const double cam_i[3] = { cams.side[I].cam.focal, cams.side[I].cam.ppx, cams.side[I].cam.ppy };
        bool have = false;
        for (int32_t J = 0; J < s.n_cams; ++J) {
            if (J == I || !((cams.valid >> J) & 1u) || row[J] < 0) continue;
            if (!have) {
                double xj[2];
                track_pixel(cams.side[J], row[J], cams.scale, xj);
                const double cam_j[3] = { cams.side[J].cam.focal, cams.side[J].cam.ppx, cams.side[J].cam.ppy };
                have = grow_point(cam_i, cam_j, cams.P[I], cams.P[J], cams.Rt[I], cams.Rt[J], xi, xj, X);
                if (have) cand |= 1u << I;
            }
            cand |= 1u << J;                             // every camera visited, before or after acceptance (:360, :391)
        }
        if (!have) return;
        s.X[3 * (size_t)t] = X[0]; s.X[3 * (size_t)t + 1] = X[1]; s.X[3 * (size_t)t + 2] = X[2];
    }
    for (int32_t J = 0; J < s.n_cams; ++J)
        if (((cand >> J) & 1u) && observation_ok(cams.Rt[J], X)) obs |= 1u << J;
    s.obs[t] = obs;
}

__global__ __launch_bounds__(kOneGroup) void grow_compact_kernel(const GrowState s, const GrowMapOut o)
{
    __shared__ uint32_t s_wave[kOneGroup / 64];
    const int32_t nt = track_count(s);
    uint32_t base = 0;
    for (int32_t t0 = 0; t0 < nt; t0 += kOneGroup) {
        const int32_t t = t0 + (int32_t)threadIdx.x;
        const uint32_t obs = t < nt ? s.obs[t] & ((1u << kMaxBatch) - 1u) : 0u;
        const bool ok = obs != 0u;
        uint32_t total;
        const uint32_t w = base + ordered_slot<kOneGroup>(ok, s_wave, &total);
        if (ok && w < (uint32_t)s.cap) {
            const int32_t c = __ffs((int)obs) - 1;       // obs.begin(): the lowest camera (colocData.hpp:112-116)
            const int32_t r = c < s.n_cams ? s.table[(size_t)t * s.n_cams + c] : -1;
            const double X0 = s.X[3 * (size_t)t], X1 = s.X[3 * (size_t)t + 1], X2 = s.X[3 * (size_t)t + 2];
            o.X[3 * (size_t)w] = X0; o.X[3 * (size_t)w + 1] = X1; o.X[3 * (size_t)w + 2] = X2;
            o.track[w] = t; o.cam[w] = c; o.row[w] = r;
            if (o.h_X) { o.h_X[3 * (size_t)w] = X0; o.h_X[3 * (size_t)w + 1] = X1; o.h_X[3 * (size_t)w + 2] = X2; }
            if (o.h_track) o.h_track[w] = t;
            if (o.h_cam) o.h_cam[w] = c;
            if (o.h_row) o.h_row[w] = r;
            if (o.h_obs) o.h_obs[w] = (uint8_t)obs;
        }
        base += total;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(o.h_n, base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

inline dim3 wide_grid(const int n) { return dim3((unsigned)((n > 0 ? n : 1) + kWide - 1) / kWide); }

} // namespace

hipError_t launch_grow_scatter(const GrowState& s, const int32_t* map_track, const double* map_X, const int n_rows, const uint32_t seed_bits,
                               hipStream_t stream)
{
    if (s.cap > 0) hipLaunchKernelGGL(grow_clear_kernel, wide_grid(s.cap), dim3(kWide), 0, stream, s);
    if (n_rows > 0) hipLaunchKernelGGL(grow_scatter_kernel, wide_grid(n_rows), dim3(kWide), 0, stream, s, map_track, map_X, (int32_t)n_rows, seed_bits);
    return hipGetLastError();
}

hipError_t launch_resect_gather(const GrowState& s, const GatherSide& side, const int camera, const ResectOut& out, hipStream_t stream)
{
    if (camera < 0 || camera >= s.n_cams) return hipErrorInvalidValue;
    Scales sc;
    level_scales(sc.v);
    hipLaunchKernelGGL(resect_gather_kernel, dim3(1), dim3(kOneGroup), 0, stream, s, side, sc, (int32_t)camera, out);
    return hipGetLastError();
}

hipError_t launch_grow(const GrowState& s, const GrowCams& cams, const int camera, const int n_tracks, hipStream_t stream)
{
    if (camera < 0 || camera >= s.n_cams) return hipErrorInvalidValue;
    if (n_tracks <= 0) return hipSuccess;
    hipLaunchKernelGGL(grow_kernel, wide_grid(n_tracks), dim3(kWide), 0, stream, s, cams, (int32_t)camera);
    return hipGetLastError();
}

hipError_t launch_grow_compact(const GrowState& s, const GrowMapOut& out, hipStream_t stream)
{
    hipLaunchKernelGGL(grow_compact_kernel, dim3(1), dim3(kOneGroup), 0, stream, s, out);
    return hipGetLastError();
}

} // namespace clc
