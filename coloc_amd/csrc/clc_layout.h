// clc_layout.h -- the layout of every workspace block of a context (not installed; no HIP).  One view per block: a plain struct of
// pointers whose carve() takes the block's arrays from a cursor in order.  That function is the ONLY statement of the layout: run on a
// measuring cursor it sizes the block, run on the allocation it places it (carve_block / place_block, clc_ctx.h).  The order and the
// counts of the arrays, every slack and the leading 64-byte word of the pinned blocks are what the kernels were written against.
// Records whose type lives in a translation unit (or in a header that needs HIP) are carved as bytes of the size the caller passes.
// A range that ONE transfer carries from pinned to device memory is a sub-layout of its own, used by both views.
#ifndef CLC_LAYOUT_H
#define CLC_LAYOUT_H

#include "clc_carve.h"
#include "acr_kind.h"

namespace clc {

struct RefineOut;          // clc_internal.h
struct InterScaleRec;

// ---- the map built on the device (map_build.hip) ----------------------------------------------------------------------------------------
// the union-find words at the head of d_mapb: [ parent | word | track_id ], up64(n_nodes) entries each
struct GraphWords {
    int32_t* parent; uint32_t* word; int32_t* track_id;
    void carve(Carve& c, size_t n_nodes)
    {
        const size_t n = up64(n_nodes);
        parent = c.take<int32_t>(n); word = c.take<uint32_t>(n); track_id = c.take<int32_t>(n);
    }
};
// d_mapb of clc_tracks_build_dev: [ union-find words | 64 ]
struct TracksDev {
    GraphWords g;
    void carve(Carve& c, size_t n_nodes) { g.carve(c, n_nodes); c.take<int32_t>(64); }
};
// d_mapb of a map build: [ union-find words | map_track capr | map_row capr | n_tracks 64 | table cap x n_cams | 64 ], capr = up64(cap)
struct MapStageDev {
    GraphWords g;
    int32_t *track, *row, *n_tracks, *table;
    void carve(Carve& c, size_t n_nodes, size_t cap, size_t n_cams)
    {
        g.carve(c, n_nodes);
        track = c.take<int32_t>(up64(cap)); row = c.take<int32_t>(up64(cap)); n_tracks = c.take<int32_t>(64);
        table = c.take<int32_t>(cap * n_cams + 64);
    }
};
// h_mapb: [ words 64 B (0: the row count, 0xFF.. = not out yet; 1: the track count) | X 3 capr | map_track capr | map_row capr |
//           table cap x n_cams | 64 ]
struct MapStagePin {
    uint32_t* words; double* X; int32_t *track, *row, *table;
    void carve(Carve& c, size_t cap, size_t n_cams)
    {
        words = c.take<uint32_t>(16); X = c.take<double>(3 * up64(cap));
        track = c.take<int32_t>(up64(cap)); row = c.take<int32_t>(up64(cap)); table = c.take<int32_t>(cap * n_cams + 64);
    }
};
// the next map's points (d_map_X_next): 3 capr doubles and 8 more
struct MapPointsDev {
    double* X;
    void carve(Carve& c, size_t rows) { X = c.take<double>(3 * rows + 8); }
};

// ---- the map grown past the seed pair (map_grow.hip) ------------------------------------------------------------------------------------
// d_growb: the per-track state [ X 3 capr | obs capr ], then the grown map's camera list [ cam capr | 64 ]
struct GrowDev {
    double* X; uint32_t* obs; int32_t* cam;
    void carve(Carve& c, size_t cap)
    {
        X = c.take<double>(3 * up64(cap)); obs = c.take<uint32_t>(up64(cap)); cam = c.take<int32_t>(up64(cap) + 64);
    }
};
// h_growb: [ row count 64 B (0xFF.. = not out yet) | camera list capr | masks capr bytes | 64 B ]
struct GrowPin {
    uint32_t* n; int32_t* cam; uint8_t* obs;
    void carve(Carve& c, size_t cap) { n = c.take<uint32_t>(16); cam = c.take<int32_t>(up64(cap)); obs = c.take<uint8_t>(up64(cap) + 64); }
};

// ---- the map replaced at the old map's scale (map_update.hip) ---------------------------------------------------------------------------
// d_align: [ match | cq | ct ], up64(n_old) entries each, and 64 more
struct AlignDev {
    int32_t *match, *cq, *ct;
    void carve(Carve& c, size_t n_old)
    {
        match = c.take<int32_t>(up64(n_old)); cq = c.take<int32_t>(up64(n_old)); ct = c.take<int32_t>(up64(n_old) + 64);
    }
};
// h_align: [ the kernel's record (64 B or its size) | X 3 n_new | match up64(n_old) + 64 ]
struct AlignPin {
    void* rec; double* X; int32_t* match;
    void carve(Carve& c, size_t n_old, size_t n_new, size_t rec_bytes, size_t rec_align)
    {
        rec = c.take_bytes(rec_bytes > 64 ? rec_bytes : 64, rec_align); X = c.take<double>(3 * n_new); match = c.take<int32_t>(up64(n_old) + 64);
    }
};

// The same two blocks of the similarity step (clc_map_align_sim_dev), for `cap` common features at most (min(n_old, the solve's capacity)):
// d_align: [ match | cq | ct as above | X_new 3 cap | X_old 3 cap of the common features: the solve's points | the transform's counter 64 B ]
struct AlignSimDev {
    AlignDev lists; double *xn, *xo; unsigned int* done;
    void carve(Carve& c, size_t n_old, size_t cap)
    {
        lists.carve(c, n_old); xn = c.take<double>(3 * cap); xo = c.take<double>(3 * cap + 8); done = c.take<unsigned int>(16, 64);
    }
};
// h_align: [ the gather's record 128 B: count word (0xFF.. = not out yet) at 0, the box of X_old at 64 | the transform's record (64 B or
//            its size) | X 3 n_new | match up64(n_old) + 64 ]
struct AlignSimPin {
    uint32_t* h_n; double* box; void* rec; double* X; int32_t* match;
    void carve(Carve& c, size_t n_old, size_t n_new, size_t rec_bytes, size_t rec_align)
    {
        h_n = c.take<uint32_t>(16, 64); box = c.take<double>(8); rec = c.take_bytes(rec_bytes > 64 ? rec_bytes : 64, rec_align);
        X = c.take<double>(3 * n_new); match = c.take<int32_t>(up64(n_old) + 64);
    }
};

// ---- the inter-camera step from device memory (inter_dev.hip) ---------------------------------------------------------------------------
// d_inter, for cap = up64(correspondences) and walk = up64(max(map rows, cap)) list entries:
//   [ Xt 3 cap | Xw 3 cap | x2f 2 cap | K 16 | Rt 12 | the refinement's record | ratio walk | term walk | corr cap | first cap |
//     cg, ck, kg, kk walk each | valid 64 | rows 64 B x cap (16-byte aligned) | match map_n + 64 | 64 B ]
struct InterDev {
    double *Xt, *Xw, *x2f, *K, *Rt, *ref, *ratio, *term;
    int32_t *corr, *first, *cg, *ck, *kg, *kk, *valid, *match;
    void* rows;                 // uint4
    void carve(Carve& c, size_t cap_in, size_t map_n, size_t ref_bytes)
    {
        const size_t cap = up64(cap_in), walk = up64(map_n > cap ? map_n : cap);
        Xt = c.take<double>(3 * cap); Xw = c.take<double>(3 * cap); x2f = c.take<double>(2 * cap); K = c.take<double>(16); Rt = c.take<double>(12);
        ref = (double*)c.take_bytes(ref_bytes, 8); ratio = c.take<double>(walk); term = c.take<double>(walk);
        corr = c.take<int32_t>(cap); first = c.take<int32_t>(cap);
        cg = c.take<int32_t>(walk); ck = c.take<int32_t>(walk); kg = c.take<int32_t>(walk); kk = c.take<int32_t>(walk); valid = c.take<int32_t>(64);
        rows = c.take_bytes(64 * cap, 16); match = c.take<int32_t>(map_n + 64);
        c.take_bytes(64, 1);
    }
};
// h_inter: [ front record 64 B | scale record (64 B or its size) | the refinement's record | 64 B ]
struct InterPin {
    int32_t* h_front; InterScaleRec* h_scale; RefineOut* h_ref;
    void carve(Carve& c, size_t scale_bytes, size_t ref_bytes)
    {
        h_front = c.take<int32_t>(16); h_scale = (InterScaleRec*)c.take_bytes(scale_bytes > 64 ? scale_bytes : 64, 8);
        h_ref = (RefineOut*)c.take_bytes(ref_bytes, 8);
        c.take_bytes(64, 1);
    }
};

// ---- a context's block of gathered correspondences (gather.hip), for `cap` of them ------------------------------------------------------
//   device [ a (a_width cap doubles) | b (2 cap) | q cap | t cap | n 64 B ]     tracks: X | x | query | map, pairs: x1 | x2 | q | t
//   pinned [ count word (64 B, 0xFF.. = not out yet) | a | b (where the points are mirrored: pairs) | q | t ]
struct GatherLayout { int a_width; bool mirror_points; };
constexpr GatherLayout kTrackLayout{ 3, false }, kPairLayout{ 2, true };
// the block as its arrays (h_a / h_b: null where the points are not mirrored).  Block: its buffers d, h and its capacity cap (GatherBlock)
struct GatherView {
    double *a, *b; int32_t *q, *t, *n; uint32_t* h_n; double *h_a = nullptr, *h_b = nullptr; int32_t *h_q, *h_t;
    GatherView() = default;
    template <class Block> GatherView(const Block& g, const GatherLayout& lay)
    {
        Carve d(g.d.ptr), h(g.h.ptr);
        dev(d, lay, g.cap); pin(h, lay, g.cap);
    }
    void dev(Carve& c, const GatherLayout& lay, size_t cap)
    {
        a = c.take<double>((size_t)lay.a_width * cap); b = c.take<double>(2 * cap);
        q = c.take<int32_t>(cap); t = c.take<int32_t>(cap); n = c.take<int32_t>(16);
    }
    void pin(Carve& c, const GatherLayout& lay, size_t cap)
    {
        h_n = c.take<uint32_t>(16);
        if (lay.mirror_points) { h_a = c.take<double>((size_t)lay.a_width * cap); h_b = c.take<double>(2 * cap); }
        h_q = c.take<int32_t>(cap); h_t = c.take<int32_t>(cap);
    }
};

// ---- the pose scratch d_pnp and its pinned staging h_pin: one layout per solve ----------------------------------------------------------
// Every array starts on 8 bytes (the blocks were laid out in doubles); what a staging launch or ONE copy carries is a sub-layout.

// The a-contrario solve (pose_batch.hip).  kind: an AcrKindId, whose row of acr_kind() gives the widths of a | b, the slots per iteration
// and the doubles per model slot; N correspondences; the records' sizes (ref_bytes: the record of what runs behind the rounds, 0:
// nothing does); batch: most iterations a round evaluates.
struct AcrDims { int kind; size_t N, state_bytes, hyp_bytes, result_bytes, ref_bytes, batch; bool points_elsewhere = false; };
// (points_elsewhere: a | b are read where the gather left them -- the similarity from device points --, the blocks hold none)
// the inputs, staged by one launch: [ a | b (a_width N | b_width N) | K1 16 | K2 16 | logc_n N + 1 floats | logc_k | state copy 0 | copy 1 = a run's start ]
struct AcrIn {
    double *a, *b, *K1, *K2; float *logc_n, *logc_k; void* state; size_t bytes;
    void carve(Carve& c, const AcrDims& d)
    {
        c.take<double>(0);
        const size_t at = c.bytes();
        const AcrKindInfo k = acr_kind(d.kind);
        a = c.take<double>(d.points_elsewhere ? 0 : (size_t)k.a_width * d.N);
        b = c.take<double>(d.points_elsewhere ? 0 : (size_t)k.b_width * d.N); K1 = c.take<double>(16); K2 = c.take<double>(16);
        logc_n = c.take<float>(d.N + 1, 8); logc_k = c.take<float>(d.N + 1, 8); state = c.take_bytes(2 * d.state_bytes, 8);
        c.take<double>(0);
        bytes = c.bytes() - at;
    }
};
// device: [ inputs | models | hypotheses | sorted lists (two copies each, by launch parity) | best inliers N | index set N | result |
//           mask N bytes | the refinement's record | 16 doubles ]
struct AcrDev {
    AcrIn in;
    double* models; void* hyp; uint32_t *sorted, *best, *index; void* result; uint8_t* mask; double* ref;
    void carve(Carve& c, const AcrDims& d)
    {
        const AcrKindInfo k = acr_kind(d.kind);
        const size_t slots = 2 * d.batch * (size_t)k.slots;                    // (the parity copies)
        in.carve(c, d);
        models = c.take<double>(slots * (size_t)k.md); hyp = c.take_bytes(d.hyp_bytes * slots, 8);
        sorted = c.take<uint32_t>(slots * d.N, 8); best = c.take<uint32_t>(d.N, 8); index = c.take<uint32_t>(d.N, 8);
        result = c.take_bytes(d.result_bytes, 8); mask = c.take<uint8_t>(d.N, 8); ref = (double*)c.take_bytes(d.ref_bytes, 8);
        c.take<double>(16);
    }
};
// pinned: [ inputs | state mirror | the polled sequence word | result | mask | inlier list N | the refinement's record | 64 B ]
struct AcrPin {
    AcrIn in;
    unsigned long long* word; void* result; uint8_t* mask; int32_t* inliers; RefineOut* ref;
    void carve(Carve& c, const AcrDims& d)
    {
        in.carve(c, d);
        c.take_bytes(2 * d.state_bytes, 8);
        word = c.take<unsigned long long>(1); result = c.take_bytes(d.result_bytes, 8); mask = c.take<uint8_t>(d.N, 8);
        inliers = c.take<int32_t>(d.N, 8); ref = (RefineOut*)c.take_bytes(d.ref_bytes, 8);
        c.take_bytes(64, 8);
    }
};
// clc_two_view_minimal: [ x1 2 N | x2 2 N | samples | models out | 8 doubles ]
struct TwoViewMinDev {
    double *x1, *x2; int32_t* samples; double* out;
    void carve(Carve& c, size_t N, size_t sample_ints, size_t out_doubles)
    {
        x1 = c.take<double>(2 * N); x2 = c.take<double>(2 * N); samples = c.take<int32_t>(sample_ints, 8); out = c.take<double>(out_doubles + 8, 8);
    }
};

// clc_sim3_minimal: [ x 3 N | y 3 N | samples 3 S | models out 12 S | 8 doubles ]
struct Sim3MinDev {
    double *x, *y; int32_t* samples; double* out;
    void carve(Carve& c, size_t N, size_t S)
    {
        x = c.take<double>(3 * N); y = c.take<double>(3 * N); samples = c.take<int32_t>(3 * S, 8); out = c.take<double>(12 * S + 8, 8);
    }
};

// One pose refinement.  Its inputs, carried by one staging launch (inter_pose.hip) or one copy (clc_pnp_refine):
// [ X 3 N | x 2 N | K 16 | Rt 12 | mask N bytes (clc_pnp_refine) ]
struct RefineIn {
    double *X, *x, *K, *Rt; uint8_t* mask; size_t bytes;
    void carve(Carve& c, size_t N, bool with_mask)
    {
        c.take<double>(0);
        const size_t at = c.bytes();
        X = c.take<double>(3 * N);
        x = c.take<double>(2 * N); K = c.take<double>(16); Rt = c.take<double>(12); mask = c.take<uint8_t>(with_mask ? N : 0);
        c.take<double>(0);
        bytes = c.bytes() - at;
    }
};
// device [ inputs | record | 8 doubles ]; pinned [ inputs | record | 64 B ], or -- overlay: the record comes back over the inputs --
// [ max(inputs, record) | 64 B ]
struct RefineDev {
    RefineIn in; void* out;
    void carve(Carve& c, size_t N, bool with_mask, size_t out_bytes) { in.carve(c, N, with_mask); out = c.take_bytes(out_bytes, 8); c.take<double>(8); }
};
struct RefinePin {
    RefineIn in; RefineOut* out;
    void carve(Carve& c, size_t N, bool with_mask, size_t out_bytes, bool overlay)
    {
        Carve o = c;
        in.carve(c, N, with_mask);
        if (overlay) { out = (RefineOut*)o.take_bytes(out_bytes, 8); if (o.bytes() > c.bytes()) c = o; }
        else out = (RefineOut*)c.take_bytes(out_bytes, 8);
        c.take_bytes(64, 8);
    }
};

// The pose from a prediction (pose_prior.hip).  What the kernel writes is pinned: [ record (64 B or its size) | mask up64(cap) bytes | 64 B ];
// the tracks are read where the gather left them (clc_track_prior_dev) or, for clc_pnp_refine_prior, come in by ONE copy:
// pinned [ X 3 N | x 2 N | record | mask | 64 B ] -> device [ X 3 N | x 2 N | 8 doubles ]
struct PriorPin {
    void* rec; uint8_t* mask;
    void carve(Carve& c, size_t cap, size_t rec_bytes)
    {
        rec = c.take_bytes(rec_bytes > 64 ? rec_bytes : 64, 8); mask = c.take<uint8_t>(up64(cap), 8);
        c.take_bytes(64, 8);
    }
};
struct PriorIn {
    double *X, *x; size_t bytes;
    void carve(Carve& c, size_t N)
    {
        c.take<double>(0);
        const size_t at = c.bytes();
        X = c.take<double>(3 * N); x = c.take<double>(2 * N);
        c.take<double>(0);
        bytes = c.bytes() - at;
    }
};
struct PriorHostDev {
    PriorIn in;
    void carve(Carve& c, size_t N) { in.carve(c, N); c.take<double>(8); }
};
struct PriorHostPin {
    PriorIn in; PriorPin out;
    void carve(Carve& c, size_t N, size_t rec_bytes) { in.carve(c, N); out.carve(c, N, rec_bytes); }
};

// The host-geometry inter-camera step's map match (inter_pose.hip): device [ idx nf | gathered rows nf x 64 B | match nm | 8 doubles ],
// pinned [ idx | match | 64 B ]; every array starts on 16 bytes
struct MapMatchDev {
    int32_t* idx; void* rows; int32_t* match;
    void carve(Carve& c, size_t nf, size_t nm)
    {
        idx = c.take<int32_t>(nf, 16); rows = c.take_bytes(64 * nf, 16); match = c.take<int32_t>(nm, 16);
        c.take<double>(8, 16);
    }
};
struct MapMatchPin {
    int32_t *idx, *match;
    void carve(Carve& c, size_t nf, size_t nm) { idx = c.take<int32_t>(nf, 16); match = c.take<int32_t>(nm, 16); c.take_bytes(64, 16); }
};

// The fixed-threshold pose entry points (capi_pose.hip).  clc_pnp_residuals / clc_pnp_score: [ Rt 12 H | X 3 N | x 2 N | K 16 | extra ]
struct PnpScoreDev {
    double *Rt, *X, *x, *K, *extra;
    void carve(Carve& c, size_t H, size_t N, size_t extra_doubles)
    {
        Rt = c.take<double>(12 * H); X = c.take<double>(3 * N); x = c.take<double>(2 * N); K = c.take<double>(16); extra = c.take<double>(extra_doubles);
    }
};
// clc_epipolar_*: [ F 9 H | x1 2 N | x2 2 N | out | 8 doubles ]
struct EpipolarDev {
    double *F, *x1, *x2, *out;
    void carve(Carve& c, size_t H, size_t N, size_t out_doubles)
    {
        F = c.take<double>(9 * H); x1 = c.take<double>(2 * N); x2 = c.take<double>(2 * N); out = c.take<double>(out_doubles + 8);
    }
};
// The RANSAC solves: `pts` doubles per correspondence, `ks` camera matrices of 16, S samples of m indices; M model slots of `md` doubles per
// sample.  Inputs, read by the first launch from pinned memory (P3P) or carried by one copy (five-point): [ points | K .. | samples ];
// outputs, one copy or the last launch's mirror: [ result record | the refinement's record | mask N bytes ]
struct RansacDims { size_t N, S, pts, ks, m, M, md, result_bytes, ref_bytes; };
struct RansacIn {
    double *pts, *K; int32_t* samples; size_t bytes;
    void carve(Carve& c, const RansacDims& d)
    {
        c.take<double>(0);
        const size_t at = c.bytes();
        pts = c.take<double>(d.pts * d.N);
        K = c.take<double>(16 * d.ks); samples = c.take<int32_t>(d.m * d.S);
        c.take<double>(0);
        bytes = c.bytes() - at;
    }
};
struct RansacOut {
    void* result; void* ref; uint8_t* mask; size_t bytes;
    void carve(Carve& c, const RansacDims& d)
    {
        c.take<double>(0);
        const size_t at = c.bytes();
        result = c.take_bytes(d.result_bytes, 8);
        ref = c.take_bytes(d.ref_bytes, 8); mask = c.take<uint8_t>(d.N, 8);
        c.take<double>(0);
        bytes = c.bytes() - at;
    }
};
// device [ inputs | models M S md | cost M S | count M S | outputs | 8 doubles ]
struct RansacDev {
    RansacIn in; double *models, *cost; int32_t* count; RansacOut out;
    void carve(Carve& c, const RansacDims& d)
    {
        in.carve(c, d);
        models = c.take<double>(d.M * d.S * d.md); cost = c.take<double>(d.M * d.S); count = c.take<int32_t>(d.M * d.S);
        out.carve(c, d);
        c.take<double>(8);
    }
};
// pinned [ inputs | outputs | 64 B ], or -- overlay: the outputs come back over the inputs -- [ max(inputs, outputs) | 64 B ]
struct RansacPin {
    RansacIn in; RansacOut out;
    void carve(Carve& c, const RansacDims& d, bool overlay)
    {
        Carve o = c;
        in.carve(c, d);
        if (overlay) { out.carve(o, d); if (o.bytes() > c.bytes()) c = o; }
        else out.carve(c, d);
        c.take_bytes(64, 8);
    }
};

// ---- the bundle adjustment (map_ba.hip) -------------------------------------------------------------------------------------------------
// d_bab, every array on 256 bytes: [ state | idx P | bits P | per-observation records P x C x rec | per-point records P x point |
//   flags 2 P | trial points 3 P | the workgroups' partial sums chunks x entries | their trial sums 4 chunks | pixels 2 P C (a composition's) ]
struct BaDims { size_t state_bytes, P, C, chunks, rec, point, entries; bool own_pixels; };      // rec / point: kBaRec / kBaPoint (ba_math.h)
struct BaDev {
    void* state; int32_t* idx; uint32_t* bits; double *rec, *pt, *flag, *X_try, *part, *tpart, *x;
    void carve(Carve& c, const BaDims& d)
    {
        state = c.take_bytes(d.state_bytes, 256); idx = c.take<int32_t>(d.P, 256); bits = c.take<uint32_t>(d.P, 256);
        rec = c.take<double>(d.P * d.C * d.rec, 256); pt = c.take<double>(d.P * d.point, 256); flag = c.take<double>(2 * d.P, 256);
        X_try = c.take<double>(3 * d.P, 256); part = c.take<double>(d.chunks * d.entries, 256); tpart = c.take<double>(4 * d.chunks, 256);
        x = c.take<double>(d.own_pixels ? 2 * d.P * d.C : 0, 256);
        c.take_bytes(0, 256);
    }
};
// h_bab: the record the host waits for
struct BaPin {
    void* rec;
    void carve(Carve& c, size_t rec_bytes) { rec = c.take_bytes(rec_bytes, 256); c.take_bytes(0, 256); }
};

// ---- the guided matches' scratch d_guided (k2nn_guided.hip) -----------------------------------------------------------------------------
// per job [ the query rows' floats (qf per row) | the train rows' points (2 per row) ], each rounded to 4 floats and starting on 16 bytes
struct GuidedDev {
    float *L, *pos;
    void carve(Carve& c, size_t qf, size_t nq, size_t nt)
    {
        L = c.take<float>((qf * nq + 3) & ~(size_t)3, 16); pos = c.take<float>((2 * nt + 3) & ~(size_t)3, 16);
    }
};

// ---- the binned map match's scratch d_binned (k2nn_binned.hip) --------------------------------------------------------------------------
// per job [ query points 2 nq floats | projections 2 nm floats | records nm x 16 B { xt, yt, row, 0 } in cell order | cell_start cells + 1 |
//           the cell of every map row nm x 2 B ], each starting on 16 bytes
struct BinnedDev {
    float *qpos, *proj; void* rec; int32_t* cell_start; uint16_t* cell_of;
    void carve(Carve& c, size_t nq, size_t nm, size_t cells)
    {
        qpos = c.take<float>((2 * nq + 3) & ~(size_t)3, 16); proj = c.take<float>((2 * nm + 3) & ~(size_t)3, 16);
        rec = c.take_bytes(16 * nm, 16); cell_start = c.take<int32_t>(cells + 1, 16); cell_of = c.take<uint16_t>(nm, 16);
    }
};

// ---- the one-to-one filter's scratch d_unique (k2nn_unique.hip) --------------------------------------------------------------------------
// per job [ claim words up64(nt) | the producer's distances up64(nq) x 2 B (a composed entry whose caller gave none) | the inverse list
//           up64(nt) (the host entry's, for the download) ], each starting on 256 bytes: the claim words of a batch are ONE range
struct UniqueDev {
    uint32_t* claim; uint16_t* best; int32_t* owner;
    void carve(Carve& c, size_t nq, size_t nt, bool with_best, bool with_owner)
    {
        claim = c.take<uint32_t>(up64(nt), 256); best = c.take<uint16_t>(with_best ? up64(nq) : 0, 256);
        owner = c.take<int32_t>(with_owner ? up64(nt) : 0, 256);
    }
};

// ---- the map extension's scratch d_extend and its pinned mirror h_extend (map_extend.hip) -----------------------------------------------
// device: [ the running row count 64 B | per job: the guided list | the masked, then one-to-one list | distances 2 B | flags 1 B | X 3 doubles,
//           up64(nq) entries each ], every array on 64 bytes
struct ExtendJobDev {
    int32_t *guided, *match; uint16_t* best; uint8_t* flag; double* X;
    void carve(Carve& c, size_t nq)
    {
        const size_t n = up64(nq);
        guided = c.take<int32_t>(n, 64); match = c.take<int32_t>(n, 64); best = c.take<uint16_t>(n, 64); flag = c.take<uint8_t>(n, 64);
        X = c.take<double>(3 * n, 64);
    }
};
struct ExtendDev {
    int32_t* rows;
    void carve(Carve& c) { rows = c.take<int32_t>(16, 64); }
};
// pinned, per job: [ the record 64 B (its first 8 bytes the polled word, 0xFF.. = not out yet) | X 3 doubles | q | t, up64(nq) entries each ]
struct ExtendJobPin {
    void* rec; double* X; int32_t *q, *t;
    void carve(Carve& c, size_t nq)
    {
        const size_t n = up64(nq);
        rec = c.take_bytes(64, 64); X = c.take<double>(3 * n, 64); q = c.take<int32_t>(n, 64); t = c.take<int32_t>(n, 64);
    }
};

// ---- the map rows' observation statistics and the cull (map_cull.hip) -------------------------------------------------------------------
// d_stat / d_stat_next: [ visible | found | last_view ], up64(cap) words each (cap = MatcherOptions.maxkp), every array on 256 bytes
struct CullStat {
    uint32_t *visible, *found, *last_view;
    void carve(Carve& c, size_t cap)
    {
        const size_t n = up64(cap);
        visible = c.take<uint32_t>(n, 256); found = c.take<uint32_t>(n, 256); last_view = c.take<uint32_t>(n, 256);
    }
};
// d_obs: the hit stamps of an observe call, [view][up64(cap)] words: a hit of the call with serial s stores s
struct ObserveDev {
    uint32_t* hit; size_t stride;
    void carve(Carve& c, size_t cap, size_t views) { stride = up64(cap); hit = c.take<uint32_t>(stride * views, 256); }
};
// d_cull: [ the record 64 B { n_kept, flagged, ratio, idle } | remap up64(rows) ]; h_cull: [ the record 64 B (its first 8 bytes the polled
// word, 0xFF.. = not out yet; then the three clause counts) | remap up64(rows) ]
struct CullDev {
    uint32_t* rec; int32_t* remap;
    void carve(Carve& c, size_t rows) { rec = c.take<uint32_t>(16, 64); remap = c.take<int32_t>(up64(rows), 64); }
};
struct CullPin {
    void* rec; int32_t* remap;
    void carve(Carve& c, size_t rows) { rec = c.take_bytes(64, 64); remap = c.take<int32_t>(up64(rows), 64); }
};

// ---- the host-pointer K2NN entries' pinned mirror h_res (capi_match.hip): [ match nq | best nq | second nq | 64 B ] --------------------
struct MatchPin {
    int32_t* match; uint16_t *best, *second;
    void carve(Carve& c, size_t nq) { match = c.take<int32_t>(nq); best = c.take<uint16_t>(nq); second = c.take<uint16_t>(nq); c.take_bytes(64, 1); }
};

} // namespace clc
#endif
