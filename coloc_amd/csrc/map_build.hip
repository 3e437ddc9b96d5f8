// map_build.hip -- the map on the device (include/coloc_hip.h: clc_tracks_build_dev, clc_map_build_dev, clc_map_init_batch_dev): what
// ColoC::initMap / updateMap (reference include/coloc/coloc.hpp:151-199, 394-459) run between filterMatches and setMapData --
// Reconstructor::initializeTracks (Reconstructor.hpp:166-173), triangulatePoints (:185-239), setupMapDatabase (colocData.hpp:89-121) --
// from the pairs' correspondences where the pair filter left them.  Launches, all enqueue-only on one stream:
//   tracks_init_kernel    every node its own root, words and track ids cleared, the track table -1
//   tracks_union_kernel   one thread per edge (blockIdx.y = pair): lock-free union-find, the LARGER root hooked under the smaller by
//                         compare-and-swap, so a component's root is its smallest node whatever the schedule
//   tracks_roots_kernel   full compression (parent = root) and, per root, the cameras seen: a camera seen twice marks the conflict
//   tracks_export_kernel  ONE workgroup: the ordered compaction of wg_compact.h over the nodes -> ids in ascending order of the root
//   tracks_table_kernel   track_feat[id][camera] = row
//   seed_triangulate_kernel  ONE workgroup: tracks with both seed cameras in id order -> get_ud_pixel (ud_pixel.h), the statements of
//                         map_math.h, the ordered compaction of the accepted points; the count last, behind the system-scope fence
//   gather_rows_kernel    (gather.hip) the map's descriptor rows, once the host knows how many; the call returns when it has run
// A build is two halves: map_stage -- everything up to the row count, the capacity check and the host outputs -- and map_install -- the
// gather into d_m and the swap of the points.  clc_map_update_batch_dev (map_update.hip) follows the same stage half with an install
// of its own, at the old map's scale.  The GROWN forms (clc_map_build_grow_dev, clc_map_init_grow_batch_dev,
// clc_map_update_grow_batch_dev) put map_stage_grown between the two halves: the resection loop over the other cameras, whose kernels
// are map_grow.hip's and whose solve is the a-contrario launch path (resect_solve, pose_batch.hip); the capacity check and the host
// outputs then describe the grown map, and the install gathers every row from the block of the camera the stage names for it.  The
// _grow_ba_ forms (map_ba.hip) bundle-adjust the per-track state behind the loop's last camera, before the rows are compacted.
// Sizes: 8 cameras x 10 k rows, 28 pairs are 80 k nodes and up to ~260 k edges.  The two single-workgroup kernels walk 80 k nodes /
// some 10 k tracks in passes of 1 024: latency-bound like the gathers, and what keeps the order a matter of one ballot per wave.
#include "clc_ctx.h"
#include "inter_geometry.h"
#include "map_math.h"
#include "ud_pixel.h"
#include "wg_compact.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

namespace clc {

namespace {

constexpr int kMapThreads = 1024;            // the two ordered compactions
constexpr int kWideThreads = 256;            // the kernels with one thread per node / edge
constexpr int kMaxPairs = CLC_MAX_TRACK_PAIRS;
constexpr uint32_t kUsed = 1u << 31, kConflict = 1u << 30, kCamBits = (1u << CLC_MAX_BATCH) - 1u;      // a node's word

struct EdgePairDev {
    int32_t cam_a, cam_b, n, n_list;
    const int32_t *q, *t, *n_dev, *index;
};
struct EdgePairs { EdgePairDev p[kMaxPairs]; };
// what every tracks kernel sees.  Node of (camera c, row r) = first[c] + r: ascending node order is (camera, row) order.
struct TrackGraph {
    int32_t n_cams, n_nodes, cap_tracks;
    int32_t first[kMaxBatch + 1];
    int32_t* parent; uint32_t* word; int32_t* track_id;      // n_nodes each
    int32_t* table; int32_t* h_table;                        // cap_tracks x n_cams (h_table: pinned mirror, nullable)
    int32_t* n_tracks;
};
struct SeedJob {
    const int32_t* table; const int32_t* n_tracks;
    int32_t n_cams, cam_i, cam_j, cap;
    GatherSide a, b;                                         // the seed cameras' 2-D sides (count unused)
    float scale[CLC_MAX_LEVELS];
    double P_i[12], P_j[12], Rt_i[12], Rt_j[12];
    double* X; int32_t* map_track; int32_t* map_row;         // out, device
    double* h_X; int32_t* h_track; int32_t* h_row;           // out, pinned mirrors (nullable)
    uint32_t* h_words;                                       // pinned { map rows, tracks }: the first comes out last
};

__device__ __forceinline__ int32_t find_root(const int32_t* parent, int32_t x)
{
    for (;;) {
        const int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ int32_t camera_of(const TrackGraph& g, const int32_t node)
{
    int32_t c = 0;
    while (c + 1 < g.n_cams && node >= g.first[c + 1]) ++c;
    return c;
}

__global__ __launch_bounds__(kWideThreads) void tracks_init_kernel(const TrackGraph g)
{
    const int32_t cells = g.cap_tracks * g.n_cams, n = g.n_nodes > cells ? g.n_nodes : cells;
    for (int32_t i = (int32_t)(blockIdx.x * kWideThreads + threadIdx.x); i < n; i += (int32_t)(gridDim.x * kWideThreads)) {
        if (i < g.n_nodes) { g.parent[i] = i; g.word[i] = 0u; g.track_id[i] = -1; }
        if (i < cells) { g.table[i] = -1; if (g.h_table) g.h_table[i] = -1; }
    }
}

__global__ __launch_bounds__(kWideThreads) void tracks_union_kernel(const TrackGraph g, const EdgePairs pairs)
{
    const EdgePairDev& p = pairs.p[blockIdx.y];
    int32_t n = p.n;
    if (p.n_dev) { const int32_t c = p.n_dev[0]; n = c < n ? (c > 0 ? c : 0) : n; }
    const int32_t e = (int32_t)(blockIdx.x * kWideThreads + threadIdx.x);
    if (e >= n) return;
    int32_t k = e;
    if (p.index) { k = p.index[e]; if (k < 0 || k >= p.n_list) return; }
    const int32_t q = p.q[k], t = p.t[k];
    if (q < 0 || q >= g.first[p.cam_a + 1] - g.first[p.cam_a] || t < 0 || t >= g.first[p.cam_b + 1] - g.first[p.cam_b]) return;
    int32_t u = g.first[p.cam_a] + q, v = g.first[p.cam_b] + t;
    g.word[u] = kUsed; g.word[v] = kUsed;               // (every writer of this launch stores the same value)
    for (;;) {
        u = find_root(g.parent, u); v = find_root(g.parent, v);
        if (u == v) break;
        const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
        // hi is a root only as long as parent[hi] == hi: whoever swaps first hooks it; the loser starts again from what it found
        if (atomicCAS(&g.parent[hi], hi, lo) == hi) break;
    }
}

__global__ __launch_bounds__(kWideThreads) void tracks_roots_kernel(const TrackGraph g)
{
    const int32_t i = (int32_t)(blockIdx.x * kWideThreads + threadIdx.x);
    if (i >= g.n_nodes || !(g.word[i] & kUsed)) return;
    const int32_t r = find_root(g.parent, i);           // (no union runs any more: the roots stand; a thread walking through node i
    __hip_atomic_store(&g.parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // meets its old parent or its root)
    const uint32_t bit = 1u << camera_of(g, i);
    if (atomicOr(&g.word[r], bit) & bit) atomicOr(&g.word[r], kConflict);
}

__global__ __launch_bounds__(kMapThreads) void tracks_export_kernel(const TrackGraph g)
{
    __shared__ uint32_t s_wave[kMapThreads / 64];
    uint32_t base = 0;
    for (int32_t i0 = 0; i0 < g.n_nodes; i0 += kMapThreads) {
        const int32_t i = i0 + (int32_t)threadIdx.x;
        const uint32_t w = i < g.n_nodes ? g.word[i] : 0u;
        const bool ok = (w & kUsed) && g.parent[i] == i && !(w & kConflict) && __popc(w & kCamBits) >= 2;      // TracksBuilder::Filter(2)
        uint32_t total;
        const uint32_t id = base + ordered_slot<kMapThreads>(ok, s_wave, &total);
        if (ok && id < (uint32_t)g.cap_tracks) g.track_id[i] = (int32_t)id;
        base += total;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) *g.n_tracks = (int32_t)(base < (uint32_t)g.cap_tracks ? base : (uint32_t)g.cap_tracks);
}

__global__ __launch_bounds__(kWideThreads) void tracks_table_kernel(const TrackGraph g)
{
    const int32_t i = (int32_t)(blockIdx.x * kWideThreads + threadIdx.x);
    if (i >= g.n_nodes || !(g.word[i] & kUsed)) return;
    const int32_t id = g.track_id[g.parent[i]];
    if (id < 0) return;
    const int32_t c = camera_of(g, i);
    const size_t cell = (size_t)id * (size_t)g.n_cams + (size_t)c;
    g.table[cell] = i - g.first[c];
    if (g.h_table) g.h_table[cell] = i - g.first[c];
}

__global__ __launch_bounds__(kMapThreads) void seed_triangulate_kernel(const SeedJob s)
{
    __shared__ uint32_t s_wave[kMapThreads / 64];
    int32_t nt = s.n_tracks[0];
    nt = nt < 0 ? 0 : nt;
    uint32_t base = 0;
    for (int32_t t0 = 0; t0 < nt; t0 += kMapThreads) {
        const int32_t t = t0 + (int32_t)threadIdx.x;
        int32_t ri = -1, rj = -1;
        if (t < nt) { ri = s.table[(size_t)t * s.n_cams + s.cam_i]; rj = s.table[(size_t)t * s.n_cams + s.cam_j]; }
        bool ok = false;
        double X[3];
        if (ri >= 0 && rj >= 0) {
            float fx, fy;
            double xi[2], xj[2];
            feature_position(s.a.kps, s.a.feat, s.a.feat_stride, (uint32_t)ri, s.scale, &fx, &fy);
            ud_pixel(fx, fy, s.a.cam, xi);
            feature_position(s.b.kps, s.b.feat, s.b.feat_stride, (uint32_t)rj, s.scale, &fx, &fy);
            ud_pixel(fx, fy, s.b.cam, xj);
            ok = seed_point(s.P_i, s.P_j, s.Rt_i, s.Rt_j, xi, xj, X);
        }
        uint32_t total;
        const uint32_t w = base + ordered_slot<kMapThreads>(ok, s_wave, &total);
        if (ok && w < (uint32_t)s.cap) {
            s.X[3 * (size_t)w] = X[0]; s.X[3 * (size_t)w + 1] = X[1]; s.X[3 * (size_t)w + 2] = X[2];
            s.map_track[w] = t; s.map_row[w] = ri;
            if (s.h_X) { s.h_X[3 * (size_t)w] = X[0]; s.h_X[3 * (size_t)w + 1] = X[1]; s.h_X[3 * (size_t)w + 2] = X[2]; }
            if (s.h_track) s.h_track[w] = t;
            if (s.h_row) s.h_row[w] = ri;
        }
        base += total;
    }
    if (threadIdx.x == 0) s.h_words[1] = (uint32_t)nt;
    // the count comes out last: the lists, the mirrors and the track count are complete and visible system-wide before it changes
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&s.h_words[0], base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// What the grow phase needs of a stage (map_stage's `detail`): where the stage left its lists, and the cameras' sides.  A stage that
// fills one leaves the capacity check and the host copies of the map's rows to the grow.
struct StageDetail {
    TrackGraph g;
    GatherSide side[kMaxBatch];
    int cam_i = 0, cam_j = 0;
    MapStageDev dev{}; MapStagePin pin{};
};
int map_stage_detail(clc_ctx* ctx, clc_map_job& job, MapStaged& out, StageDetail* detail);

// a tracks job, validated, as the kernels take it.  *edge_rows: the widest pair (the union launch's grid)
int tracks_inputs(clc_ctx* ctx, const clc_tracks_job& job, TrackGraph& g, EdgePairs& ep, int* edge_rows, const char* who)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, (std::string(who) + what).c_str()); };
    if (job.n_cams < 2 || job.n_cams > kMaxBatch) return bad(": n_cams must be 2 .. CLC_MAX_BATCH");
    if (job.n_pairs < 0 || job.n_pairs > kMaxPairs || (job.n_pairs > 0 && !job.pairs)) return bad(": n_pairs must be 0 .. CLC_MAX_TRACK_PAIRS");
    g = TrackGraph{};
    ep = EdgePairs{};
    g.n_cams = job.n_cams;
    size_t nodes = 0, edges = 0;
    for (int c = 0; c < job.n_cams; ++c) {
        if (job.rows[c] < 0) return bad(": negative row capacity");
        g.first[c] = (int32_t)nodes;
        nodes += (size_t)job.rows[c];
        if (nodes > ((size_t)1 << 28)) return bad(": too many rows");
    }
    for (int c = job.n_cams; c <= kMaxBatch; ++c) g.first[c] = (int32_t)nodes;
    g.n_nodes = (int32_t)nodes;
    *edge_rows = 0;
    for (int p = 0; p < job.n_pairs; ++p) {
        const clc_tracks_pair& in = job.pairs[p];
        if (in.cam_a < 0 || in.cam_a >= in.cam_b || in.cam_b >= job.n_cams) return bad(": a pair needs 0 <= cam_a < cam_b < n_cams");
        if (in.n < 0 || (in.n > 0 && (!in.d_q || !in.d_t)) || (in.d_index && in.n_list < 0)) return bad(": a pair's lists");
        if (((uintptr_t)in.d_q | (uintptr_t)in.d_t | (uintptr_t)in.d_n | (uintptr_t)in.d_index) & 3u) return bad(": misaligned device pointer");
        ep.p[p] = EdgePairDev{ in.cam_a, in.cam_b, in.n, in.d_index ? in.n_list : in.n, in.d_q, in.d_t, in.d_n, in.d_index };
        edges += (size_t)in.n;
        *edge_rows = std::max(*edge_rows, in.n);
    }
    // every track holds an edge of its own and two nodes of its own
    g.cap_tracks = (int32_t)std::min(edges, nodes / 2);
    return CLC_OK;
}

void graph_words(TrackGraph& g, const GraphWords& w) { g.parent = w.parent; g.word = w.word; g.track_id = w.track_id; }

// the host copies of a staged map's lists, n rows, out of the pinned block
void map_lists_out(clc_map_job& job, const MapStagePin& pin, const uint32_t n)
{
    if (job.map_track && n) memcpy(job.map_track, pin.track, sizeof(int32_t) * n);
    if (job.map_row && n) memcpy(job.map_row, pin.row, sizeof(int32_t) * n);
    if (job.X && n) memcpy(job.X, pin.X, sizeof(double) * 3 * n);
}

hipError_t launch_tracks(const TrackGraph& g, const EdgePairs& ep, const int n_pairs, const int edge_rows, hipStream_t st)
{
    const auto blocks = [](const size_t n) { return dim3((unsigned)std::max<size_t>(1, (n + kWideThreads - 1) / kWideThreads)); };
    const size_t cells = (size_t)g.cap_tracks * (size_t)g.n_cams;
    hipLaunchKernelGGL(tracks_init_kernel, blocks(std::min<size_t>(std::max((size_t)g.n_nodes, cells), (size_t)1 << 20)), dim3(kWideThreads), 0, st, g);
    if (n_pairs > 0 && edge_rows > 0)
        hipLaunchKernelGGL(tracks_union_kernel, dim3(blocks((size_t)edge_rows).x, (unsigned)n_pairs), dim3(kWideThreads), 0, st, g, ep);
    hipLaunchKernelGGL(tracks_roots_kernel, blocks((size_t)g.n_nodes), dim3(kWideThreads), 0, st, g);
    hipLaunchKernelGGL(tracks_export_kernel, dim3(1), dim3(kMapThreads), 0, st, g);
    hipLaunchKernelGGL(tracks_table_kernel, blocks((size_t)g.n_nodes), dim3(kWideThreads), 0, st, g);
    return hipGetLastError();
}

} // namespace

// The STAGE half of a map build: tracks, the seed launch, the wait for the row count, the capacity check, the host outputs.  On CLC_OK
// the new map's points lie in d_map_X_next and its row list in the map block (out.d_row); the context's map is as it was.
int map_stage(clc_ctx* ctx, clc_map_job& job, MapStaged& out) { return map_stage_detail(ctx, job, out, nullptr); }

namespace {

int map_stage_detail(clc_ctx* ctx, clc_map_job& job, MapStaged& out, StageDetail* detail)
{
    out = MapStaged{};
    ctx->grow_table = nullptr;                           // (the block the last grown build's table lies in is rewritten)
    job.n_tracks = 0; job.map_n = 0; job.status = CLC_OK;
    if (!ctx->has_mat) return job.status = fail(ctx, CLC_ERR_STATE, "map_build: context created without matcher options");
    TrackGraph g; EdgePairs ep; int edge_rows = 0;
    int rc = tracks_inputs(ctx, job.tracks, g, ep, &edge_rows, "map_build");
    if (rc != CLC_OK) return job.status = rc;
    if (job.seed_pair < 0 || job.seed_pair >= job.tracks.n_pairs) return job.status = fail(ctx, CLC_ERR_BAD_ARG, "map_build: seed_pair is not one of the pairs");
    GatherSide side[kMaxBatch];
    for (int c = 0; c < job.tracks.n_cams; ++c) {
        const clc_map_camera& m = job.cams[c];
        rc = gather_side(ctx, "map_build", nullptr, m.d_kps, m.d_feat, m.feat_stride, m.cam, side[c]);
        if (rc != CLC_OK) return job.status = rc;
        if ((uintptr_t)m.d_desc & 15u) return job.status = fail(ctx, CLC_ERR_BAD_ARG, "map_build: misaligned device pointer");
    }
    const int cam_i = job.tracks.pairs[job.seed_pair].cam_a, cam_j = job.tracks.pairs[job.seed_pair].cam_b;
    if (!job.cams[cam_i].d_desc && job.tracks.rows[cam_i] > 0) return job.status = fail(ctx, CLC_ERR_BAD_ARG, "map_build: the lower seed camera needs its descriptor block");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the map block and its pinned mirror (MapStageDev, MapStagePin); the next map's points apart
    const size_t cap = (size_t)g.cap_tracks, n_cams = (size_t)g.n_cams;
    MapStageDev dev; MapStagePin pin; MapPointsDev next;
    rc = carve_block(ctx, ctx->d_mapb, 1, 4, true, "growing the map block", [&](Carve& c) { dev.carve(c, (size_t)g.n_nodes, cap, n_cams); });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_map_X_next, 1, 4, true, "growing the next map's points", [&](Carve& c) { next.carve(c, up64(cap)); });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->h_mapb, 1, 4, true, "growing the pinned map block", [&](Carve& c) { pin.carve(c, cap, n_cams); });
    if (rc != CLC_OK) return job.status = rc;
    graph_words(g, dev.g);
    int32_t* d_track = dev.track; int32_t* d_row = dev.row;
    g.n_tracks = dev.n_tracks; g.table = dev.table;
    uint32_t* h_words = pin.words;
    g.h_table = job.track_feat ? pin.table : nullptr;
    SeedJob s{};
    s.table = g.table; s.n_tracks = g.n_tracks; s.n_cams = g.n_cams; s.cam_i = cam_i; s.cam_j = cam_j; s.cap = g.cap_tracks;
    s.a = side[cam_i]; s.b = side[cam_j];
    level_scales(s.scale);
    memcpy(s.Rt_i, job.Rt_seed_a, sizeof s.Rt_i); memcpy(s.Rt_j, job.Rt_seed_b, sizeof s.Rt_j);
    projective_equivalent(side[cam_i].cam.focal, side[cam_i].cam.ppx, side[cam_i].cam.ppy, s.Rt_i, s.P_i);
    projective_equivalent(side[cam_j].cam.focal, side[cam_j].cam.ppx, side[cam_j].cam.ppy, s.Rt_j, s.P_j);
    s.X = next.X; s.map_track = d_track; s.map_row = d_row;
    s.h_X = job.X ? pin.X : nullptr; s.h_track = job.map_track ? pin.track : nullptr; s.h_row = job.map_row ? pin.row : nullptr;
    if (detail) { s.h_X = nullptr; s.h_track = nullptr; s.h_row = nullptr; }      // (the grown map's rows go out instead)
    s.h_words = h_words;
    __atomic_store_n(&h_words[0], 0xFFFFFFFFu, __ATOMIC_RELAXED);
    // behind whatever produced the inputs: an event on the producer's stream, no host synchronisation
    hipStream_t prod = (hipStream_t)job.after_stream;
    if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));
    CLC_HIP(ctx, launch_tracks(g, ep, job.tracks.n_pairs, edge_rows, st));
    hipLaunchKernelGGL(seed_triangulate_kernel, dim3(1), dim3(kMapThreads), 0, st, s);
    CLC_HIP(ctx, hipGetLastError());
    // the one number the host needs
    rc = wait_pinned(ctx, &h_words[0], 0xFFFFFFFFu, st, std::chrono::steady_clock::now(), 2, "map_build: the seed launch left no count");
    if (rc != CLC_OK) return job.status = rc;
    const uint32_t n = __atomic_load_n(&h_words[0], __ATOMIC_ACQUIRE);
    job.n_tracks = (int)h_words[1];
    if (job.track_feat && job.n_tracks > 0) memcpy(job.track_feat, pin.table, sizeof(int32_t) * (size_t)job.n_tracks * (size_t)g.n_cams);
    if (detail) {
        detail->g = g; detail->cam_i = cam_i; detail->cam_j = cam_j; detail->dev = dev; detail->pin = pin;
        memcpy(detail->side, side, sizeof side);
        out.n = (int)std::min<uint32_t>(n, (uint32_t)g.cap_tracks); out.cam_i = cam_i; out.cam_j = cam_j; out.d_row = d_row;
        return CLC_OK;
    }
    if (n > ctx->mopts.maxkp) return job.status = fail(ctx, CLC_ERR_CAPACITY, "map_build: more map rows than MatcherOptions.maxkp (the previous map stays)");
    map_lists_out(job, pin, n);
    job.map_n = (int)n;
    out.n = (int)n; out.cam_i = cam_i; out.cam_j = cam_j; out.d_row = d_row;
    return CLC_OK;
}

} // namespace

// The INSTALL half (clc_map_build_dev, clc_map_init_batch_dev): the staged map becomes the context's.
int map_install(clc_ctx* ctx, clc_map_job& job, const MapStaged& staged)
{
    const uint32_t n = (uint32_t)staged.n;
    const int cam_i = staged.cam_i;
    const int32_t* d_row = staged.d_row;
    hipStream_t st = ctx->stream;
    map_rows_replaced(ctx);
    if (n == 0) { ctx->map_n = 0; ctx->map_X_n = -1; return CLC_OK; }
    // install: the points change places with the previous map's (whatever read those was enqueued on this stream before), the
    // descriptor rows are gathered from the lower seed camera's block straight into the matcher's map.  The map is published only
    // once the gather has run, as clc_set_map publishes behind its upload: the context's stream is non-blocking, so a matcher call
    // on ANOTHER stream straight after this one would otherwise sweep rows still being written, and a caller that describes its next
    // frame into the seed camera's block would change rows still being read.  (Some microseconds of device work, no data moved.)
    ctx->map_n = -1; ctx->map_X_n = -1;
    hipError_t e;
    if (staged.d_cam) {
        // a grown map: every row from the block of the lowest camera that observes its landmark
        RowSources srcs{};
        for (int c = 0; c < job.tracks.n_cams; ++c) srcs.src[c] = (const uint4*)job.cams[c].d_desc;
        e = launch_gather_rows_multi(srcs, staged.d_cam, d_row, ctx->d_m.as<uint4>(), n, st);
    } else e = launch_gather_rows((const uint4*)job.cams[cam_i].d_desc, d_row, ctx->d_m.as<uint4>(), n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return job.status = fail(ctx, CLC_ERR_HIP, "map_build: gathering the map's descriptors", e);
    std::swap(ctx->d_map_X, ctx->d_map_X_next);
    ctx->map_n = (int)n; ctx->map_X_n = (int)n;
    return CLC_OK;
}

namespace {

int map_build(clc_ctx* ctx, clc_map_job& job)
{
    MapStaged staged;
    const int rc = map_stage(ctx, job, staged);
    return rc == CLC_OK ? map_install(ctx, job, staged) : rc;
}

void grow_outputs_none(clc_map_grow& gr)
{
    for (int c = 0; c < kMaxBatch; ++c) {
        gr.resected[c] = 0; gr.status[c] = CLC_GROW_OK; gr.n_corr[c] = 0; gr.n_inliers[c] = 0; gr.error_max[c] = 0.0;
        memset(gr.Rt[c], 0, sizeof gr.Rt[c]);
    }
    gr.n_seed_rows = 0; gr.n_added = 0;
}

// The STAGE half of a grown build: map_stage, then -- between it and the install -- the resection loop of reconstructScene
// (Reconstructor.hpp:153-154) on the per-track state and the grown map's rows.  Per camera the host waits for the resection count and
// for the solve's rounds, as every a-contrario solve does; after the last camera for one more word, the grown map's row count.
int map_stage_grown(clc_ctx* ctx, clc_map_job& job, clc_map_grow& gr, MapStaged& out, clc_map_ba* ba = nullptr)
{
    grow_outputs_none(gr);
    if (gr.max_iteration < 0) return job.status = fail(ctx, CLC_ERR_BAD_ARG, "map_grow: negative max_iteration");
    if (job.tracks.n_cams >= 2 && job.tracks.n_cams <= kMaxBatch)
        for (int c = 0; c < job.tracks.n_cams; ++c)
            if (!job.cams[c].d_desc && job.tracks.rows[c] > 0) return job.status = fail(ctx, CLC_ERR_BAD_ARG, "map_grow: every camera needs its descriptor block");
    StageDetail d;
    int rc = map_stage_detail(ctx, job, out, &d);
    if (rc != CLC_OK) return rc;
    const int n_cams = d.g.n_cams, nt = job.n_tracks, n_seed = out.n;
    hipStream_t st = ctx->stream;
    gr.n_seed_rows = n_seed;
    memcpy(gr.Rt[d.cam_i], job.Rt_seed_a, sizeof gr.Rt[0]); memcpy(gr.Rt[d.cam_j], job.Rt_seed_b, sizeof gr.Rt[0]);
    // the per-track state and the grown map's camera list (GrowDev), their pinned mirror (GrowPin)
    GrowDev gd; GrowPin gp;
    rc = carve_block(ctx, ctx->d_growb, 1, 4, true, "growing the map grow block", [&](Carve& c) { gd.carve(c, (size_t)d.g.cap_tracks); });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->h_growb, 1, 4, true, "growing the pinned map grow block", [&](Carve& c) { gp.carve(c, (size_t)d.g.cap_tracks); });
    // the resection lists: at most one entry per row of the camera, and the solve takes 16 384
    int widest = 1;
    for (int c = 0; c < n_cams; ++c) widest = std::max(widest, job.tracks.rows[c]);
    if (rc == CLC_OK) rc = ensure_gather(ctx, ctx->trk, (size_t)std::min(widest, kAcrMaxN), kTrackLayout);
    if (rc != CLC_OK) return job.status = rc;
    GrowState s{};
    s.table = d.g.table; s.n_tracks = d.g.n_tracks; s.n_cams = n_cams; s.cap = d.g.cap_tracks;
    s.X = gd.X; s.obs = gd.obs;
    int32_t* d_cam = gd.cam;
    uint32_t* h_n = gp.n;
    GrowCams cams{};
    memcpy(cams.side, d.side, sizeof cams.side);
    level_scales(cams.scale);
    const auto set_pose = [&](const int c, const double* Rt) {
        memcpy(cams.Rt[c], Rt, sizeof cams.Rt[c]);
        projective_equivalent(cams.side[c].cam.focal, cams.side[c].cam.ppx, cams.side[c].cam.ppy, cams.Rt[c], cams.P[c]);
        cams.valid |= 1u << c;
    };
    set_pose(d.cam_i, job.Rt_seed_a);
    set_pose(d.cam_j, job.Rt_seed_b);
    hipError_t e = launch_grow_scatter(s, d.dev.track, ctx->d_map_X_next.as<double>(), n_seed, (1u << d.cam_i) | (1u << d.cam_j), st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return job.status = fail(ctx, CLC_ERR_HIP, "map_grow: the scatter launch", e); }
    const GatherView v(ctx->trk, kTrackLayout);
    const int block_cap = (int)std::min<size_t>(ctx->trk.cap, (size_t)kAcrMaxN);
    int k = 0;
    for (int I = 0; I < n_cams; ++I) {
        if (I == d.cam_i || I == d.cam_j) continue;
        const uint64_t seed = gr.seed + (uint64_t)k++;
        // step 1: the resection list into the context's track block, its count into the block's pinned word
        __atomic_store_n(v.h_n, 0xFFFFFFFFu, __ATOMIC_RELAXED);
        const ResectOut ro{ v.a, v.b, v.q, v.t, v.h_q, v.h_t, v.n, v.h_n, block_cap };
        e = launch_resect_gather(s, cams.side[I], I, ro, st);
        if (e != hipSuccess) { (void)hipStreamSynchronize(st); return job.status = fail(ctx, CLC_ERR_HIP, "map_grow: the resect gather launch", e); }
        rc = wait_pinned(ctx, v.h_n, 0xFFFFFFFFu, st, std::chrono::steady_clock::now(), 2, "map_grow: the resect gather left no count");
        if (rc != CLC_OK) return job.status = rc;
        const uint32_t N = __atomic_load_n(v.h_n, __ATOMIC_ACQUIRE);
        gr.n_corr[I] = (int)N;
        if (N == 0) { gr.status[I] = CLC_GROW_NO_TRACKS; continue; }                       // Reconstructor.hpp:274-277
        if (N > (uint32_t)kAcrMaxN) { gr.status[I] = CLC_GROW_CAPACITY; continue; }         // (nothing is truncated silently)
        // step 2: SfM_Localizer::Localize(P3P_KE_CVPR17): the a-contrario solve, success iff more than 2.5 x 3 inliers
        rc = resect_solve(ctx, (int)N, job.cams[I].cam, gr.max_iteration > 0 ? gr.max_iteration : 256, seed, gr.precision, gr.Rt[I], &gr.n_inliers[I],
                          &gr.error_max[I]);
        if (rc != CLC_OK) return job.status = rc;
        if (!(gr.n_inliers[I] > 2.5 * 3)) { gr.status[I] = CLC_GROW_NO_POSE; continue; }     // DEVIATION: skipped, not stored (:316)
        gr.resected[I] = 1;
        // step 3: the camera is valid; its tracks gain it or are triangulated against the valid cameras
        set_pose(I, gr.Rt[I]);
        e = launch_grow(s, cams, I, nt, st);
        if (e != hipSuccess) { (void)hipStreamSynchronize(st); return job.status = fail(ctx, CLC_ERR_HIP, "map_grow: the grow launch", e); }
    }
    // refinePose (Reconstructor.hpp:160-161; map_ba.hip): the valid cameras' poses and the landmarks X[t] adjusted where they lie.  obs is
    // not written, so every discrete output below is the one of a build without the step.
    if (ba) {
        BaProblem pb{};
        pb.n_cams = n_cams; pb.n_points = std::max(0, std::min(nt, (int)s.cap)); pb.mask = cams.valid;
        for (int c = 0; c < n_cams; ++c) {
            pb.K[c][0] = cams.side[c].cam.focal; pb.K[c][1] = cams.side[c].cam.ppx; pb.K[c][2] = cams.side[c].cam.ppy;
            memcpy(pb.Rt[c], cams.Rt[c], sizeof pb.Rt[c]);
        }
        pb.X = s.X; pb.obs = s.obs; pb.x = nullptr; pb.cams = &cams; pb.table = s.table;
        rc = ba_drive(ctx, pb, *ba);
        if (rc != CLC_OK) return job.status = rc;
        for (int c = 0; c < n_cams; ++c)
            if ((cams.valid >> c) & 1u) memcpy(gr.Rt[c], pb.Rt[c], sizeof gr.Rt[c]);
        memcpy(job.Rt_seed_a, pb.Rt[d.cam_i], sizeof job.Rt_seed_a); memcpy(job.Rt_seed_b, pb.Rt[d.cam_j], sizeof job.Rt_seed_b);
    }
    // setupMapDatabase over the landmarks: the rows in track-id order, over the staged seed map's lists
    __atomic_store_n(h_n, 0xFFFFFFFFu, __ATOMIC_RELAXED);
    GrowMapOut mo{};
    mo.X = ctx->d_map_X_next.as<double>(); mo.track = d.dev.track; mo.cam = d_cam; mo.row = d.dev.row;
    mo.h_X = job.X ? d.pin.X : nullptr; mo.h_track = job.map_track ? d.pin.track : nullptr; mo.h_row = job.map_row ? d.pin.row : nullptr;
    mo.h_cam = gr.map_cam ? gp.cam : nullptr; mo.h_obs = gr.map_obs ? gp.obs : nullptr; mo.h_n = h_n;
    e = launch_grow_compact(s, mo, st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return job.status = fail(ctx, CLC_ERR_HIP, "map_grow: the compaction launch", e); }
    rc = wait_pinned(ctx, h_n, 0xFFFFFFFFu, st, std::chrono::steady_clock::now(), 2, "map_grow: the compaction left no count");
    if (rc != CLC_OK) return job.status = rc;
    const uint32_t n = __atomic_load_n(h_n, __ATOMIC_ACQUIRE);
    ctx->grow_table = s.table; ctx->grow_n_tracks = s.n_tracks; ctx->grow_n_cams = n_cams; ctx->grow_cap = s.cap;
    if (n > ctx->mopts.maxkp) return job.status = fail(ctx, CLC_ERR_CAPACITY, "map_grow: more map rows than MatcherOptions.maxkp (the previous map stays)");
    map_lists_out(job, d.pin, n);
    if (gr.map_cam && n) memcpy(gr.map_cam, gp.cam, sizeof(int32_t) * n);
    if (gr.map_obs && n) memcpy(gr.map_obs, gp.obs, n);
    job.map_n = (int)n;
    gr.n_added = (int)n - n_seed;
    out.n = (int)n; out.d_cam = d_cam;
    return CLC_OK;
}

} // namespace

int map_build_grow(clc_ctx* ctx, clc_map_job& job, clc_map_grow& gr, clc_map_ba* ba)
{
    MapStaged staged;
    const int rc = map_stage_grown(ctx, job, gr, staged, ba);
    return rc == CLC_OK ? map_install(ctx, job, staged) : rc;
}

// The seven batch compositions (their extern "C" entries side by side below): the filters, the selection, the seed poses and the stage
// half are ONE path; what the optional steps change is the stage half (grown, bundle-adjusted) and what follows it -- the install above,
// or a replacement rule of map_update.hip.  Which steps go together is checked HERE, ahead of the first write to an out field of grow,
// align or sim (ba_check clears ba's own as it checks, as it did in the entries).
int map_init_batch(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, const MapSteps& steps)
{
    clc_map_grow* const gr = steps.grow; clc_map_ba* const ba = steps.ba;
    clc_map_align* const align = steps.align; clc_map_align_sim* const sim = steps.sim;
    if ((ba && !gr) || (align && sim)) return CLC_ERR_BAD_ARG;
    if (ba && ba_check(nullptr, ba, "map_init_batch") != CLC_OK) return CLC_ERR_BAD_ARG;
    if (gr) grow_outputs_none(*gr);
    if (sim) sim_outputs_none(*sim);
    if (align) align_outputs_none(*align);
    if (n_pairs < 1 || n_pairs > kMaxPairs || !ctxs || !pair_jobs || !job) return CLC_ERR_BAD_ARG;
    const int rc0 = check_batch_contexts(ctxs, n_pairs, "map_init_batch: every pair needs a context of its own");
    if (rc0 != CLC_OK) return rc0;
    clc_ctx* c0 = ctxs[0];
    if (align || sim) { const int rs = map_align_state(c0, "map_update_batch"); if (rs != CLC_OK) return job->status = rs; }
    job->seed_pair = -1; job->n_tracks = 0; job->map_n = -1; job->status = CLC_OK;
    memset(job->entered, 0, sizeof job->entered);
    if (job->tracks.n_pairs != n_pairs || !job->tracks.pairs) return job->status = fail(c0, CLC_ERR_BAD_ARG, "map_init_batch: tracks.pairs must name the cameras of every pair job");
    // 1. the pair gathers and the five-point filters, exactly as clc_pair_filter_batch_dev runs them; the vote needs E, the inlier
    //    list and the undistorted pixels on the host (the pinned mirrors): where the caller did not ask for them they land here
    const size_t np = (size_t)n_pairs;
    std::vector<clc_pair_job> pj(pair_jobs, pair_jobs + np);
    std::vector<std::vector<double>> Es(np), x1s(np), x2s(np);
    std::vector<std::vector<int32_t>> inls(np);
    for (size_t p = 0; p < np; ++p) {
        const size_t room = (size_t)std::max(pj[p].nq, 1);
        if (!pj[p].M) { Es[p].assign(9, 0.0); pj[p].M = Es[p].data(); }
        if (!pj[p].x1) { x1s[p].assign(2 * room, 0.0); pj[p].x1 = x1s[p].data(); }
        if (!pj[p].x2) { x2s[p].assign(2 * room, 0.0); pj[p].x2 = x2s[p].data(); }
        if (!pj[p].inliers) { inls[p].assign(room, 0); pj[p].inliers = inls[p].data(); }
    }
    std::vector<const int32_t*> d_inl(np, nullptr);
    const int worst = pair_filter_essential(ctxs, pj.data(), n_pairs, d_inl.data());
    for (size_t p = 0; p < np; ++p) {
        clc_pair_job& o = pair_jobs[p]; const clc_pair_job& r = pj[p];
        o.n_pairs = r.n_pairs; o.n_inliers = r.n_inliers; o.iterations = r.iterations; o.status = r.status; o.error_max = r.error_max; o.min_nfa = r.min_nfa;
    }
    if (worst != CLC_OK) return job->status = worst;
    // 2. who enters, and the seed: strictly the most inliers, the first in pair order (Reconstructor.hpp:112-118)
    std::vector<clc_tracks_pair> tp(np);
    std::vector<InterFront> votes(np);
    int seed = -1, most = 0;
    for (size_t p = 0; p < np; ++p) {
        const clc_pair_job& r = pj[p];
        tp[p] = clc_tracks_pair{ job->tracks.pairs[p].cam_a, job->tracks.pairs[p].cam_b, nullptr, nullptr, 0, nullptr, nullptr, 0 };
        if (r.n_inliers < 13 || !d_inl[p]) continue;                                     // 2.5 x 5
        const double K1[9] = { r.cam_a.focal, 0, r.cam_a.ppx, 0, r.cam_a.focal, r.cam_a.ppy, 0, 0, 1 };
        const double K2[9] = { r.cam_b.focal, 0, r.cam_b.ppx, 0, r.cam_b.focal, r.cam_b.ppy, 0, 0, 1 };
        clc_inter_pose_job v{};
        v.tv.x1 = r.x1; v.tv.x2 = r.x2; v.tv.n = r.n_pairs; v.tv.K1 = K1; v.tv.K2 = K2; v.tv.E = r.M; v.tv.inliers = r.inliers; v.tv.n_inliers = r.n_inliers;
        if (inter_relative(v, votes[p]) != CLC_INTER_OK) continue;
        const GatherView gv(ctxs[p]->pair, kPairLayout);
        tp[p].d_q = gv.q; tp[p].d_t = gv.t; tp[p].n = r.n_inliers; tp[p].d_index = d_inl[p];
        tp[p].n_list = std::min(r.n_pairs, (int)ctxs[p]->pair.cap);
        job->entered[p] = 1;
        if (r.n_inliers > most) { most = r.n_inliers; seed = (int)p; }
    }
    if (seed < 0) return CLC_OK;
    double Crel[3];
    pose_center(votes[(size_t)seed].R, votes[(size_t)seed].t, Crel);
    seed_poses(job->origin_R, job->origin_C, votes[(size_t)seed].R, Crel, job->scale, job->Rt_seed_a, job->Rt_seed_b);
    // 3. clc_map_build_dev on ctxs[0]; the pair blocks were written on its stream and the inlier lists are out (the filters returned)
    const clc_tracks_pair* callers = job->tracks.pairs;
    void* const after = job->after_stream;
    job->tracks.pairs = tp.data(); job->seed_pair = seed; job->after_stream = nullptr;
    MapStaged staged;
    int rc = gr ? map_stage_grown(c0, *job, *gr, staged, ba) : map_stage(c0, *job, staged);
    if (rc == CLC_OK) rc = sim ? map_align_sim_staged(c0, *job, staged, *sim, gr) : (align ? map_align_staged(c0, *job, staged, *align, gr) : map_install(c0, *job, staged));
    job->tracks.pairs = callers; job->after_stream = after;
    // (the union launch read the other contexts' blocks and pinned lists; it ran before the count the build waited for came out)
    return rc;
}

} // namespace clc

using namespace clc;

extern "C" {

int clc_tracks_build_dev(clc_ctx* ctx, const clc_tracks_job* job, int32_t* d_track_feat, int32_t* d_n_tracks, void* stream)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "tracks_build: null context / job");
    TrackGraph g; EdgePairs ep; int edge_rows = 0;
    int rc = tracks_inputs(ctx, *job, g, ep, &edge_rows, "tracks_build");
    if (rc != CLC_OK) return rc;
    if (!d_n_tracks || (g.cap_tracks > 0 && !d_track_feat)) return fail(ctx, CLC_ERR_BAD_ARG, "tracks_build: null output");
    if (((uintptr_t)d_track_feat | (uintptr_t)d_n_tracks) & 3u) return fail(ctx, CLC_ERR_BAD_ARG, "tracks_build: misaligned device pointer");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    TracksDev dev;
    rc = carve_block(ctx, ctx->d_mapb, 1, 4, true, "growing the map block", [&](Carve& c) { dev.carve(c, (size_t)g.n_nodes); });
    if (rc != CLC_OK) return rc;
    graph_words(g, dev.g);
    g.table = d_track_feat; g.h_table = nullptr; g.n_tracks = d_n_tracks;
    ctx->grow_table = nullptr;                           // (the block the last grown build's table lies in is rewritten)
    CLC_HIP(ctx, launch_tracks(g, ep, job->n_pairs, edge_rows, pick(ctx, stream)));
    return CLC_OK;
}

int clc_map_build_dev(clc_ctx* ctx, clc_map_job* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "map_build: null context / job");
    return map_build(ctx, *job);
}

int clc_map_build_grow_dev(clc_ctx* ctx, clc_map_job* job, clc_map_grow* grow)
{
    if (!ctx || !job || !grow) return fail(ctx, CLC_ERR_BAD_ARG, "map_build_grow: null context / job / grow");
    return map_build_grow(ctx, *job, *grow, nullptr);
}

// ---- the seven batch compositions: each names the steps it REQUIRES; every other rule is map_init_batch's (MapSteps: grow, ba, align, sim)
int clc_map_init_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job)
{
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{});
}

int clc_map_init_grow_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_grow* grow)
{
    if (!grow) return CLC_ERR_BAD_ARG;
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{ grow });
}

int clc_map_init_grow_ba_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_grow* grow, clc_map_ba* ba)
{
    if (!grow || !ba) return CLC_ERR_BAD_ARG;
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{ grow, ba });
}

int clc_map_update_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align* align)
{
    if (!align) return CLC_ERR_BAD_ARG;
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{ nullptr, nullptr, align });
}

int clc_map_update_grow_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align* align, clc_map_grow* grow)
{
    if (!align || !grow) return CLC_ERR_BAD_ARG;
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{ grow, nullptr, align });
}

int clc_map_update_grow_ba_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align* align, clc_map_grow* grow,
                                     clc_map_ba* ba)
{
    if (!align || !grow || !ba) return CLC_ERR_BAD_ARG;
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{ grow, ba, align });
}

int clc_map_update_sim_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align_sim* sim,
                                 clc_map_grow* grow, clc_map_ba* ba)
{
    if (!sim) return CLC_ERR_BAD_ARG;
    return map_init_batch(ctxs, pair_jobs, n_pairs, job, MapSteps{ grow, ba, nullptr, sim });
}

int clc_map_resect_build_dev(clc_ctx* ctx, const clc_map_job* job, int camera, double* d_X, double* d_x, int32_t* d_track, int32_t* d_row, int32_t* d_n,
                             void* stream)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "map_resect_build: null context / job");
    if (job->tracks.n_cams < 2 || job->tracks.n_cams > kMaxBatch || camera < 0 || camera >= job->tracks.n_cams)
        return fail(ctx, CLC_ERR_BAD_ARG, "map_resect_build: camera must be one of the job's cameras");
    if (!ctx->grow_table || ctx->grow_n_cams != job->tracks.n_cams)
        return fail(ctx, CLC_ERR_STATE, "map_resect_build: the context holds no per-track state of a grown build with that many cameras");
    const clc_map_camera& m = job->cams[camera];
    GatherSide side;
    int rc = gather_side(ctx, "map_resect_build", nullptr, m.d_kps, m.d_feat, m.feat_stride, m.cam, side);
    if (rc != CLC_OK) return rc;
    if (job->tracks.rows[camera] < 0 || !d_n || (job->tracks.rows[camera] > 0 && (!d_X || !d_x))) return fail(ctx, CLC_ERR_BAD_ARG, "map_resect_build: null output");
    if (((uintptr_t)d_X & 7u) || ((uintptr_t)d_x & 7u) || ((uintptr_t)d_track & 3u) ||
        ((uintptr_t)d_row & 3u) || ((uintptr_t)d_n & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "map_resect_build: misaligned device pointer");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    GrowState s{};
    s.table = ctx->grow_table; s.n_tracks = ctx->grow_n_tracks; s.n_cams = ctx->grow_n_cams; s.cap = ctx->grow_cap;
    // the per-track state where the grown build left it: its view placed again, refused if the block no longer holds it
    GrowDev gd;
    rc = place_block(ctx, ctx->d_growb, "map_resect_build: the grow block does not hold the last grown build's state", [&](Carve& c) { gd.carve(c, (size_t)s.cap); });
    if (rc != CLC_OK) return rc;
    s.X = gd.X; s.obs = gd.obs;
    const ResectOut ro{ d_X, d_x, d_track, d_row, nullptr, nullptr, d_n, nullptr, job->tracks.rows[camera] };
    CLC_HIP(ctx, launch_resect_gather(s, side, camera, ro, pick(ctx, stream)));
    return CLC_OK;
}

} // extern "C"
