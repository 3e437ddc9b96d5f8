// k2nn_proj.h -- what the two map matches around a predicted pose share (not installed): the sweep with the gate in its loop
// (k2nn_guided.hip: clc_match_map_guided_dev) and the match through a cell grid (k2nn_binned.hip: clc_match_map_binned_dev).  The prep
// launch, its records and the argument checks live in k2nn_guided.hip as they stood; the grid's translation unit calls them.
#ifndef CLC_K2NN_PROJ_H
#define CLC_K2NN_PROJ_H

#include "clc_ctx.h"

#include <vector>

namespace clc {

// The map match's prep records: the frame's rows and camera, the predicted [R|t]; the landmarks are the context's, the same for every job.
struct ProjPrepJob {
    GatherSide a;
    double Rt[12];
    uint32_t nq, pad_;
    float* qpos; float* proj;         // the context's scratch: 2 nq / 2 nm floats
    float* qpos_out; float* proj_out; // the caller's copies, nullable
};
struct ProjPrepList {
    ProjPrepJob j[kMaxBatch];
    const double* map_X; uint32_t nm; // the landmarks of the map rows (d_map_X), nm = the context's map rows
    float scale[CLC_MAX_LEVELS];      // as PairJobs::scale
};
static_assert(sizeof(ProjPrepList) <= 4096, "ProjPrepList is passed as a kernel argument: a batch of CLC_MAX_BATCH cameras is ONE prep launch");

// every check of clc_match_map_guided_dev / _batch_dev, before anything is enqueued: the context's state, each job's arguments (its 2-D
// side into sides[j]) and the 2^22 rows a key's index holds
int proj_checks(clc_ctx* ctx, const clc_map_guided_job* jobs, int n_jobs, std::vector<GatherSide>& sides);
// proj_prep_kernel over n jobs of at most `rows` rows (query rows + map rows) each
hipError_t proj_prep_launch(const ProjPrepList& prep, uint32_t rows, int n, hipStream_t st);
// clc_match_map_guided_batch_dev behind its extern "C" name
int proj_batch(clc_ctx* ctx, const clc_map_guided_job* jobs, int n_jobs, void* stream);

} // namespace clc
#endif
