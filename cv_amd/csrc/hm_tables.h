// hm_tables.h — the tables the matcher's expand and k-NN kernels read (hm_match.hip), one entry per blockIdx.y.  They are written
// by the host (push_recoded of hm_match.hip) or on the device (k_vp_tables of hm_view_plan.hip): one layout, stated here.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/akz.h"

struct HmProb {            // one (queries -> targets) problem
    const uint4* q;        // query descriptors (4 x uint4 each)
    const uint32_t* nq;    // device count
    uint32_t q_cap;
    const uint4* t;
    const uint32_t* nt;
    uint32_t t_cap;
    akz_neighbor* out;     // [q_cap][2]
};

struct HmExpandJob {
    const uint32_t* src;   // [cap][16] descriptor words
    const uint32_t* count; // device count
    uint32_t cap;
    uint32_t* dst;         // [cap][128] words of +-1 bytes
};

struct HmProbX {           // like HmProb, on the +-1 recoded descriptors
    const uint32_t* q;     // [q_cap][128] words
    const uint32_t* nq;
    uint32_t q_cap;
    const uint32_t* t;
    const uint32_t* nt;
    uint32_t t_cap;
    akz_neighbor* out;
};

// A search whose tables are written on the device (hm_view_plan.hip) and launched by hm_match.hip, which owns the kernels:
// hm_internal_planned(c, s, false) stages the host list `iq`, grows d_exp to (n_frames + exp_blocks) * cap * words and says
// where the tables go and which family the context searches with; (c, s, true) launches the expand over n_frames + exp_blocks
// jobs and the k-NN search over n_probs problems, grids from these rooms alone.
struct HmPlannedSearch {
    // in
    const uint32_t* iq;        // host [n_frames]
    uint32_t n_frames, exp_blocks, n_probs, cap;
    int k;
    const HmExpandJob* jobs;   // device [n_frames + exp_blocks]     (for the launch)
    const void* probs;         // device [n_probs] HmProbX, or HmProb when `valu`
    // out of the preparation
    const uint32_t* d_iq;      // the staged copy of iq
    uint32_t* exp;             // d_exp
    uint32_t words;            // per recoded descriptor: 64 (FP4) or 128 (int8)
    bool valu;                 // the VALU kernel on the descriptors as they are: no recoding, HmProb
};
struct hm_ctx;
int32_t hm_internal_planned(hm_ctx* c, HmPlannedSearch* s, bool launch);
