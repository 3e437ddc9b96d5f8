// acr_kind.h -- the models of the a-contrario path (acransac.hip, pose_batch.hip), each stated ONCE (not installed; plain C++17, no HIP).
// What a kind IS -- its sample, its slots, the widths of its points, what it needs from the caller, its NFA exponent, when a batch of it
// goes lockstep -- is a row of acr_kind(); what a kind DOES differently (its residual, its alpha, what runs behind its rounds, how its
// model leaves) is one switch over AcrKindId with a case per kind at the site.  A new kind: a row here, and every such switch stops
// compiling until it has its case.  Device code reads the table in constant expressions only.
#ifndef CLC_ACR_KIND_H
#define CLC_ACR_KIND_H

#include "../../include/coloc_hip.h"

namespace clc {

// the values AcrProblem::kind carries
enum AcrKindId : int {
    kAcrResection = 0,      // P3P, [R|t]: a = X, b = x, K1 (Localizer::localizeImage)
    kAcrEssential = 1,      // five-point, {F, E}: a = x1, b = x2 in pixels, K1 / K2, image 2 (RobustMatcher::filterEssential)
    kAcrFundamental = 2,    // seven-point, F: a = x1, b = x2, conditioned by the image size (filterFundamental)
    kAcrHomography = 3,     // four-point, H: as F (filterHomography)
    kAcrSimilarity = 4,     // three points, [sR|t] NEW -> OLD: a = X_new, b = X_old, no camera, no image (sim3_math.h)
    kAcrKindCount = 5
};

struct AcrKindInfo {
    int m, M, md;                 // sample size; most models per sample; doubles per model slot
    int a_width, b_width;         // doubles per correspondence in a | b
    int slots;                    // model slots per iteration in the workspace, between the parity copies
    bool needs_K1, needs_K2, needs_image;
    bool conditioned;             // the points enter as x * d + t of the image size (ACKernelAdaptor's NormalizePoints)
    bool in_place;                // points in device memory are read where they lie -- with their box from the caller --, not staged
    double mult;                  // the NFA exponent: error^mult
    bool error_in_units;          // the reported error is sqrt(e) / norm; else e as it is
    int lockstep_from, lockstep_cap;      // smallest batch that goes lockstep by default; iterations per round of a lockstep batch
};

constexpr AcrKindInfo acr_kind(const int kind)
{
    switch (kind) {
    //                             m   M  md   a  b  slots  K1     K2     image  cond   place  mult units  lockstep
    case kAcrResection:   return { 3,  4, 12,  3, 2,  4,    true,  false, false, false, false, 1.0, true,  8,  8 };
    case kAcrEssential:   return { 5, 10, 18,  2, 2, 10,    true,  true,  true,  false, false, 0.5, false, 4, 12 };
    case kAcrFundamental: return { 7,  3, 12,  2, 2,  4,    false, false, true,  true,  false, 0.5, true,  8,  8 };
    case kAcrHomography:  return { 4,  1, 12,  2, 2,  4,    false, false, true,  true,  false, 1.0, true,  8,  8 };
    case kAcrSimilarity:  return { 3,  1, 12,  3, 3,  4,    false, false, false, false, true,  1.5, true,  8,  8 };
    }
    return {};
}
constexpr bool acr_is_kind(const int kind) { return (unsigned)kind < (unsigned)kAcrKindCount; }

// what the code around the table was written against: clc_acr_sample draws <= 8 indices, AcrState::model / AcrResult::model hold 18
// doubles, a sample's models lie in its iteration's slots, and the one-launch round (acr_round_body, every kind but the essential, whose
// round is two launches) strides its workspace by 4 slots of 12 doubles per iteration
constexpr bool acr_kinds_fit()
{
    for (int k = 0; k < kAcrKindCount; ++k) {
        const AcrKindInfo i = acr_kind(k);
        if (i.m < 1 || i.m > 8 || i.md > 18 || i.M < 1 || i.M > i.slots) return false;
        if (k != kAcrEssential && (i.slots != 4 || i.md != 12)) return false;
    }
    return true;
}
static_assert(acr_kinds_fit(), "a kind outgrows the sampler, the model record or its slots");

// RobustMatcher's model letter -> the kind (colocParams::model, RobustMatcher.hpp:399-405); -1: none
constexpr int acr_kind_of_model(const int clc_model)
{
    return clc_model == CLC_MODEL_ESSENTIAL ? kAcrEssential : (clc_model == CLC_MODEL_FUNDAMENTAL ? kAcrFundamental : (clc_model == CLC_MODEL_HOMOGRAPHY ? kAcrHomography : -1));
}

} // namespace clc
#endif
