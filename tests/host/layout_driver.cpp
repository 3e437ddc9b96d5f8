// Every workspace view of coloc_amd/csrc/clc_layout.h on the host, under ASan + UBSan (tests/test_layout_host.py): measured with a cursor
// without a base, placed on an allocation of exactly that size, every array written over its full stated extent with a byte of its own
// and read back.  A layout whose measuring and placing runs disagree, whose arrays overrun the block or overlap, or whose pointers are
// less aligned than their type's rule fails here.  The extents below restate what the kernels and copies use; they are not read from
// the header.
#include "clc_carve.h"
#include "clc_layout.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

using namespace clc;

namespace {

struct Arr { const char* name; void* p; size_t bytes, align; int group; };      // arrays of different groups may overlay each other
using Arrs = std::vector<Arr>;
int g_cases = 0;

[[noreturn]] void die(const char* view, const char* what, const char* arr = "")
{
    fprintf(stderr, "FAIL %s: %s %s\n", view, what, arr);
    exit(1);
}

template <class T> Arr arr(const char* name, T* p, size_t count, size_t align = alignof(T), int group = 0) { return Arr{ name, (void*)p, count * sizeof(T), align, group }; }
Arr raw(const char* name, void* p, size_t bytes, size_t align, int group = 0) { return Arr{ name, p, bytes, align, group }; }

// lay(cursor, arrays): carves the view and lists its arrays
void check(const char* view, const std::function<void(Carve&, Arrs&)>& lay)
{
    ++g_cases;
    Arrs a;
    Carve measure;
    lay(measure, a);
    for (const Arr& x : a) if (x.p) die(view, "a measuring cursor handed out a pointer", x.name);
    const size_t need = measure.bytes();
    if (need == 0) return;
    void* block = nullptr;
    if (posix_memalign(&block, 256, need) != 0) die(view, "allocation");          // exactly `need` bytes: ASan sees every overrun
    a.clear();
    Carve place(block);
    lay(place, a);
    if (place.bytes() != need) die(view, "measure and place disagree");
    int groups = 0;
    for (const Arr& x : a) {
        if (!x.p) die(view, "null pointer", x.name);
        if ((uintptr_t)x.p % x.align) die(view, "misaligned", x.name);
        if ((uint8_t*)x.p < (uint8_t*)block || (uint8_t*)x.p + x.bytes > (uint8_t*)block + need) die(view, "outside the block", x.name);
        groups = x.group + 1 > groups ? x.group + 1 : groups;
    }
    for (int g = 0; g < groups; ++g) {
        for (size_t i = 0; i < a.size(); ++i) if (a[i].group == g) memset(a[i].p, (int)(i + 1), a[i].bytes);
        for (size_t i = 0; i < a.size(); ++i) {
            if (a[i].group != g) continue;
            const uint8_t* p = (const uint8_t*)a[i].p;
            for (size_t k = 0; k < a[i].bytes; ++k) if (p[k] != (uint8_t)(i + 1)) die(view, "overwritten by a later array", a[i].name);
        }
    }
    free(block);
}

// one transfer carries the range: every member at the same offset from the first in both views
void same_offsets(const char* view, std::initializer_list<const void*> dev, std::initializer_list<const void*> pin, size_t dev_bytes, size_t pin_bytes)
{
    if (dev.size() != pin.size() || dev_bytes != pin_bytes) die(view, "shared range differs in size");
    auto d = dev.begin(); auto p = pin.begin();
    for (; d != dev.end(); ++d, ++p)
        if ((const uint8_t*)*d - (const uint8_t*)*dev.begin() != (const uint8_t*)*p - (const uint8_t*)*pin.begin()) die(view, "shared range differs between the device and the pinned view");
}

const size_t kCounts[] = { 0, 1, 63, 64, 65, 1000 };
const size_t kCams[] = { 2, 8 };
const size_t kRecs[] = { 1, 64, 200 };

void map_views()
{
    for (size_t nodes : kCounts) {
        check("TracksDev", [&](Carve& c, Arrs& a) {
            TracksDev v; v.carve(c, nodes);
            a = { arr("parent", v.g.parent, nodes), arr("word", v.g.word, nodes), arr("track_id", v.g.track_id, nodes) };
        });
        for (size_t cap : kCounts) for (size_t cams : kCams) {
            check("MapStageDev", [&](Carve& c, Arrs& a) {
                MapStageDev v; v.carve(c, nodes, cap, cams);
                a = { arr("parent", v.g.parent, nodes), arr("word", v.g.word, nodes), arr("track_id", v.g.track_id, nodes), arr("track", v.track, up64(cap)),
                      arr("row", v.row, up64(cap)), arr("n_tracks", v.n_tracks, 64), arr("table", v.table, cap * cams) };
            });
        }
    }
    for (size_t cap : kCounts) {
        for (size_t cams : kCams)
            check("MapStagePin", [&](Carve& c, Arrs& a) {
                MapStagePin v; v.carve(c, cap, cams);
                a = { arr("words", v.words, 16, 64), arr("X", v.X, 3 * up64(cap)), arr("track", v.track, up64(cap)), arr("row", v.row, up64(cap)),
                      arr("table", v.table, cap * cams) };
            });
        check("MapPointsDev", [&](Carve& c, Arrs& a) { MapPointsDev v; v.carve(c, cap); a = { arr("X", v.X, 3 * cap + 8) }; });
        check("GrowDev", [&](Carve& c, Arrs& a) {
            GrowDev v; v.carve(c, cap);
            a = { arr("X", v.X, 3 * up64(cap)), arr("obs", v.obs, up64(cap)), arr("cam", v.cam, up64(cap)) };
        });
        check("GrowPin", [&](Carve& c, Arrs& a) {
            GrowPin v; v.carve(c, cap);
            a = { arr("n", v.n, 16, 64), arr("cam", v.cam, up64(cap)), arr("obs", v.obs, up64(cap)) };
        });
        check("AlignDev", [&](Carve& c, Arrs& a) {
            AlignDev v; v.carve(c, cap);
            a = { arr("match", v.match, up64(cap)), arr("cq", v.cq, up64(cap)), arr("ct", v.ct, up64(cap)) };
        });
        for (size_t n_new : kCounts) for (size_t rec : kRecs)
            check("AlignPin", [&](Carve& c, Arrs& a) {
                AlignPin v; v.carve(c, cap, n_new, rec, 8);
                a = { raw("rec", v.rec, rec < 64 ? 64 : rec, 8), arr("X", v.X, 3 * n_new), arr("match", v.match, up64(cap)) };
            });
    }
}

void inter_views()
{
    for (size_t n : kCounts) for (size_t map_n : kCounts) for (size_t rec : kRecs)
        check("InterDev", [&](Carve& c, Arrs& a) {
            InterDev v; v.carve(c, n, map_n, rec);
            const size_t cap = up64(n), walk = up64(map_n > cap ? map_n : cap);
            a = { arr("Xt", v.Xt, 3 * cap), arr("Xw", v.Xw, 3 * cap), arr("x2f", v.x2f, 2 * cap), arr("K", v.K, 16), arr("Rt", v.Rt, 12), raw("ref", v.ref, rec, 8),
                  arr("ratio", v.ratio, walk), arr("term", v.term, walk), arr("corr", v.corr, cap), arr("first", v.first, cap), arr("cg", v.cg, walk),
                  arr("ck", v.ck, walk), arr("kg", v.kg, walk), arr("kk", v.kk, walk), arr("valid", v.valid, 64), raw("rows", v.rows, 64 * cap, 16),
                  arr("match", v.match, map_n) };
        });
    for (size_t scale : kRecs) for (size_t rec : kRecs)
        check("InterPin", [&](Carve& c, Arrs& a) {
            InterPin v; v.carve(c, scale, rec);
            a = { arr("front", v.h_front, 16, 64), raw("scale", v.h_scale, scale < 64 ? 64 : scale, 8), raw("ref", v.h_ref, rec, 8) };
        });
}

void gather_views()
{
    for (const GatherLayout& lay : { kTrackLayout, kPairLayout }) for (size_t cap : kCounts) {
        check("GatherView device", [&](Carve& c, Arrs& a) {
            GatherView v; v.dev(c, lay, cap);
            a = { arr("a", v.a, (size_t)lay.a_width * cap), arr("b", v.b, 2 * cap), arr("q", v.q, cap), arr("t", v.t, cap), arr("n", v.n, 16) };
        });
        check("GatherView pinned", [&](Carve& c, Arrs& a) {
            GatherView v; v.pin(c, lay, cap);
            a = { arr("h_n", v.h_n, 16, 64), arr("h_q", v.h_q, cap), arr("h_t", v.h_t, cap) };
            if (lay.mirror_points) { a.push_back(arr("h_a", v.h_a, (size_t)lay.a_width * cap)); a.push_back(arr("h_b", v.h_b, 2 * cap)); }
            else if (c.base && (v.h_a || v.h_b)) die("GatherView pinned", "points mirrored where the layout has none");
        });
    }
}

// the five kinds of the a-contrario solve as the kernels and copies use them (resection, E, F, H, similarity): doubles per correspondence
// in a | b, model slots per iteration, doubles per model slot -- written out here, not read from acr_kind()
const size_t kAcrA[5] = { 3, 2, 2, 2, 3 }, kAcrB[5] = { 2, 2, 2, 2, 3 }, kAcrSlots[5] = { 4, 10, 4, 4, 4 }, kAcrMd[5] = { 12, 18, 12, 12, 12 };

void acr_in_arrays(const AcrIn& in, const AcrDims& d, Arrs& a)
{
    const size_t n_pts = d.points_elsewhere ? 0 : d.N;              // (points read where they lie: zero-length a | b)
    a = { arr("a", in.a, kAcrA[d.kind] * n_pts), arr("b", in.b, kAcrB[d.kind] * n_pts), arr("K1", in.K1, 16), arr("K2", in.K2, 16),
          arr("logc_n", in.logc_n, d.N + 1, 8), arr("logc_k", in.logc_k, d.N + 1, 8), raw("state", in.state, 2 * d.state_bytes, 8) };
}

void pose_views()
{
    // (only the similarity reads device points in place)
    for (int kind = 0; kind < 5; ++kind) for (int elsewhere = 0; elsewhere < (kind == 4 ? 2 : 1); ++elsewhere)
    for (int refine = 0; refine < 2; ++refine) for (size_t N : kCounts) for (size_t rec : kRecs) {
        const AcrDims d{ kind, N, rec, rec, rec, refine ? rec : 0, 128, elsewhere != 0 };
        const size_t slots = 2 * 128 * kAcrSlots[kind];
        const size_t* md = kAcrMd;
        AcrDev dv{}; AcrPin pv{};
        check("AcrDev", [&](Carve& c, Arrs& a) {
            dv.carve(c, d);
            acr_in_arrays(dv.in, d, a);
            if (elsewhere && c.base && (dv.in.a != dv.in.b || (void*)dv.in.b != (void*)dv.in.K1)) die("AcrDev", "points elsewhere, yet a | b take room");
            for (const Arr& x : Arrs{ arr("models", dv.models, slots * md[kind]), raw("hyp", dv.hyp, rec * slots, 8), arr("sorted", dv.sorted, slots * N, 8),
                                      arr("best", dv.best, N, 8), arr("index", dv.index, N, 8), raw("result", dv.result, rec, 8), arr("mask", dv.mask, N, 8),
                                      raw("ref", dv.ref, refine ? rec : 0, 8) })
                a.push_back(x);
        });
        check("AcrPin", [&](Carve& c, Arrs& a) {
            pv.carve(c, d);
            acr_in_arrays(pv.in, d, a);
            for (const Arr& x : Arrs{ arr("word", pv.word, 1), raw("result", pv.result, rec, 8), arr("mask", pv.mask, N, 8), arr("inliers", pv.inliers, N, 8),
                                      raw("ref", pv.ref, refine ? rec : 0, 8) })
                a.push_back(x);
        });
        // (the views stand as the last, placing run left them; their blocks are gone, the addresses are only subtracted)
        same_offsets("AcrIn", { dv.in.a, dv.in.b, dv.in.K1, dv.in.K2, dv.in.logc_n, dv.in.logc_k, dv.in.state },
                     { pv.in.a, pv.in.b, pv.in.K1, pv.in.K2, pv.in.logc_n, pv.in.logc_k, pv.in.state }, dv.in.bytes, pv.in.bytes);
        // the staging launch moves an even number of doubles: the blocks go on past it
        if (dv.in.bytes % 8) die("AcrIn", "the staged range is no whole number of doubles");
    }
    for (size_t N : kCounts) for (size_t S : kCounts)
        check("TwoViewMinDev", [&](Carve& c, Arrs& a) {
            TwoViewMinDev v; v.carve(c, N, 7 * S, 27 * S);
            a = { arr("x1", v.x1, 2 * N), arr("x2", v.x2, 2 * N), arr("samples", v.samples, 7 * S, 8), arr("out", v.out, 27 * S) };
        });
    for (size_t N : kCounts) for (int mask = 0; mask < 2; ++mask) for (size_t rec : kRecs) {
        RefineDev dv{};
        check("RefineDev", [&](Carve& c, Arrs& a) {
            dv.carve(c, N, mask != 0, rec);
            a = { arr("X", dv.in.X, 3 * N), arr("x", dv.in.x, 2 * N), arr("K", dv.in.K, 16), arr("Rt", dv.in.Rt, 12), arr("mask", dv.in.mask, mask ? N : 0),
                  raw("out", dv.out, rec, 8) };
        });
        for (int overlay = 0; overlay < 2; ++overlay) {
            RefinePin pv{};
            check("RefinePin", [&](Carve& c, Arrs& a) {
                pv.carve(c, N, mask != 0, rec, overlay != 0);
                a = { arr("X", pv.in.X, 3 * N), arr("x", pv.in.x, 2 * N), arr("K", pv.in.K, 16), arr("Rt", pv.in.Rt, 12), arr("mask", pv.in.mask, mask ? N : 0),
                      raw("out", pv.out, rec, 8, overlay) };
            });
            same_offsets("RefineIn", { dv.in.X, dv.in.x, dv.in.K, dv.in.Rt, dv.in.mask }, { pv.in.X, pv.in.x, pv.in.K, pv.in.Rt, pv.in.mask }, dv.in.bytes, pv.in.bytes);
        }
    }
    for (size_t nf : kCounts) for (size_t nm : kCounts) {
        check("MapMatchDev", [&](Carve& c, Arrs& a) {
            MapMatchDev v; v.carve(c, nf, nm);
            a = { arr("idx", v.idx, nf, 16), raw("rows", v.rows, 64 * nf, 16), arr("match", v.match, nm, 16) };
        });
        check("MapMatchPin", [&](Carve& c, Arrs& a) {
            MapMatchPin v; v.carve(c, nf, nm);
            a = { arr("idx", v.idx, nf, 16), arr("match", v.match, nm, 16) };
        });
    }
    for (size_t H : kCounts) for (size_t N : kCounts) {
        check("PnpScoreDev", [&](Carve& c, Arrs& a) {
            PnpScoreDev v; v.carve(c, H, N, H * N);
            a = { arr("Rt", v.Rt, 12 * H), arr("X", v.X, 3 * N), arr("x", v.x, 2 * N), arr("K", v.K, 16), arr("extra", v.extra, H * N) };
        });
        check("EpipolarDev", [&](Carve& c, Arrs& a) {
            EpipolarDev v; v.carve(c, H, N, 2 * H);
            a = { arr("F", v.F, 9 * H), arr("x1", v.x1, 2 * N), arr("x2", v.x2, 2 * N), arr("out", v.out, 2 * H) };
        });
    }
    // P3P: 5 doubles per correspondence, one K, samples of 3, 4 slots of 12; five-point: 4, two K, samples of 5, 10 slots of 18
    for (int five = 0; five < 2; ++five) for (size_t N : kCounts) for (size_t S : kCounts) for (size_t rec : kRecs) for (int refine = 0; refine < 2; ++refine) {
        const RansacDims d = five ? RansacDims{ N, S, 4, 2, 5, 10, 18, rec, 0 } : RansacDims{ N, S, 5, 1, 3, 4, 12, rec, refine ? rec : 0 };
        const auto in_arrays = [&](const RansacIn& in, Arrs& a) {
            a = { arr("pts", in.pts, d.pts * N), arr("K", in.K, 16 * d.ks), arr("samples", in.samples, d.m * S) };
        };
        const auto out_arrays = [&](const RansacOut& out, Arrs& a, int group) {
            a.push_back(raw("result", out.result, rec, 8, group)); a.push_back(raw("ref", out.ref, d.ref_bytes, 8, group));
            a.push_back(arr("mask", out.mask, N, 8, group));
        };
        RansacDev dv{};
        check("RansacDev", [&](Carve& c, Arrs& a) {
            dv.carve(c, d);
            in_arrays(dv.in, a);
            a.push_back(arr("models", dv.models, d.M * S * d.md)); a.push_back(arr("cost", dv.cost, d.M * S)); a.push_back(arr("count", dv.count, d.M * S));
            out_arrays(dv.out, a, 0);
        });
        RansacPin pv{};
        check("RansacPin", [&](Carve& c, Arrs& a) {
            pv.carve(c, d, five != 0);
            in_arrays(pv.in, a);
            out_arrays(pv.out, a, five);
        });
        same_offsets("RansacIn", { dv.in.pts, dv.in.K, dv.in.samples }, { pv.in.pts, pv.in.K, pv.in.samples }, dv.in.bytes, pv.in.bytes);
        same_offsets("RansacOut", { dv.out.result, dv.out.ref, dv.out.mask }, { pv.out.result, pv.out.ref, pv.out.mask }, dv.out.bytes, pv.out.bytes);
    }
}

void other_views()
{
    for (size_t P : kCounts) for (size_t C : kCams) for (size_t rec : kRecs) for (int own = 0; own < 2; ++own) {
        if (P == 0) continue;                                        // (the driver adjusts max(points, 1))
        const size_t chunks = (P + 127) / 128, entries = 6 * C * (6 * C + 1) / 2 + 6 * C + 3;
        check("BaDev", [&](Carve& c, Arrs& a) {
            BaDev v; v.carve(c, BaDims{ rec, P, C, chunks, 21, 9, entries, own != 0 });
            a = { raw("state", v.state, rec, 256), arr("idx", v.idx, P, 256), arr("bits", v.bits, P, 256), arr("rec", v.rec, P * C * 21, 256),
                  arr("pt", v.pt, P * 9, 256), arr("flag", v.flag, 2 * P, 256), arr("X_try", v.X_try, 3 * P, 256), arr("part", v.part, chunks * entries, 256),
                  arr("tpart", v.tpart, 4 * chunks, 256), arr("x", v.x, own ? 2 * P * C : 0, 256) };
            if (c.bytes() % 256) die("BaDev", "the block is no multiple of 256 bytes");
        });
    }
    for (size_t rec : kRecs) check("BaPin", [&](Carve& c, Arrs& a) { BaPin v; v.carve(c, rec); a = { raw("rec", v.rec, rec, 256) }; });
    // two jobs behind each other, the lines' 3 floats per query row or the map match's 2
    for (size_t qf : { (size_t)3, (size_t)2 }) for (size_t nq : kCounts) for (size_t nt : kCounts)
        check("GuidedDev", [&](Carve& c, Arrs& a) {
            GuidedDev v[2];
            v[0].carve(c, qf, nq, nt); v[1].carve(c, qf, nt, nq);
            a = { arr("L0", v[0].L, qf * nq, 16), arr("pos0", v[0].pos, 2 * nt, 16), arr("L1", v[1].L, qf * nt, 16), arr("pos1", v[1].pos, 2 * nq, 16) };
        });
    for (size_t nq : kCounts)
        check("MatchPin", [&](Carve& c, Arrs& a) {
            MatchPin v; v.carve(c, nq);
            a = { arr("match", v.match, nq), arr("best", v.best, nq), arr("second", v.second, nq) };
        });
}

} // namespace

int main()
{
    map_views();
    inter_views();
    gather_views();
    pose_views();
    other_views();
    printf("layout ok: %d cases\n", g_cases);
    return 0;
}
