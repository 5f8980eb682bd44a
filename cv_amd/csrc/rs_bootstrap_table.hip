// rs_bootstrap_table.hip — the two integer steps around the three-view bootstrap that create a reconstruction on gfx950: the join
// (and shuffle) of VSlam::init_reconstruction (cv-sfm/src/lib.rs:992-999, 1190-1191, 1216, 1234) in front of
// rs_three_view_init_batch_device and VSlamData::add_reconstruction with add_view / add_landmark (lib.rs:377-500) behind it, out
// of place.  Integer data movement; every decision is include/akz_bootstrap_table_math.h, the text the CPU checker
// (tests/cpp/bootstrap_table_host.c) compiles too — parity: host build == HIP, byte for byte.
//
// rs_join_pairs_batch_device is one kernel:
//   k_jp_join        one workgroup per scene.  The two maps centre feature -> position of its LAST entry live in LDS (atomicMax
//                    on the position: the bytes do not depend on arrival order); three ordered compactions (akz_block_scan) give
//                    the triples in the order of the first list and the one-pair lists in the order of their own; with
//                    RS_BATCH_SHUFFLE the triples wait in scratch and leave in the stable order of their keys
//                    (lds_radix_sort_ids, in the LDS the maps no longer need).
// rs_add_reconstruction_batch_device, in stream order:
//   k_bt_check_table one lane per start of the existing table and of its reconstruction ranges.
//   k_bt_old         the existing table goes to the outputs unchanged: one lane per row copies its list (and gives the row's key
//                    to d_landmarks_out); a refused table is copied word for word.
//   k_bt_validate    one workgroup per scene: not accepted, valid or refused; the maps centre feature -> first / second feature
//                    and the used features of the two other frames (atomicCAS: a feature in two accepted matches refuses).
//   k_bt_accept      ONE lane walks the scenes in order: a valid scene none of whose frames an earlier accepted scene names is
//                    accepted; its row and observation bases, the ranges, the constraint's views and verdict, the totals.
//   k_bt_copy        the keypoint blocks, counts and poses of the accepted scenes, and the constraint's poses.
//   k_bt_rows        the rows of the centre features: a workgroup per tile of kTblTile rows of a scene adds the lengths in front of
//                    its tile, scans its own and writes starts, lengths and lists.
//   k_bt_new_rows    one workgroup per scene: the features of the first, then the second frame in no accepted match, compacted in
//                    feature order, one row each (their starts are arithmetic).
//   k_tbl_tail       (rs_table.h) every start behind the filled rows equals the total, every count there is 0.
// Nothing here waits on a value another workgroup has yet to write: the levels are separate launches; every loop is bounded by
// an argument of the call or a checked count.
#include "rs_table.h"
#include "../../include/akz_bootstrap_table_math.h"

namespace {

constexpr int kJpBlock = 1024;                               // lds_radix_sort_ids' block
constexpr int kJpWaves = kJpBlock / 64;
constexpr uint32_t kKpWords = sizeof(akz_keypoint) / sizeof(uint32_t);
static_assert(sizeof(akz_keypoint) % sizeof(uint32_t) == 0, "keypoint blocks are copied word by word");

static_assert(RS_JP_OK == AKZ_JP_OK && RS_JP_NO_MODEL == AKZ_JP_NO_MODEL && RS_JP_FEW_INLIERS == AKZ_JP_FEW_INLIERS &&
              RS_JP_BAD_INDEX == AKZ_JP_BAD_INDEX, "the join's verdicts");
static_assert(RS_AR_OK == AKZ_AR_OK && RS_AR_NOT_ACCEPTED == AKZ_AR_NOT_ACCEPTED && RS_AR_BAD_INDEX == AKZ_AR_BAD_INDEX &&
              RS_AR_TAKEN == AKZ_AR_TAKEN && RS_AR_BAD_TABLE == AKZ_AR_BAD_TABLE, "verdicts");
static_assert(RS_AR_S_TRIPLES == AKZ_AR_S_TRIPLES && RS_AR_S_FIRST == AKZ_AR_S_FIRST && RS_AR_S_SECOND == AKZ_AR_S_SECOND &&
              RS_AR_S_LANDMARKS == AKZ_AR_S_LANDMARKS && RS_AR_STATS == AKZ_AR_STATS && RS_AR_COUNTS == AKZ_AR_COUNTS, "stats words");
static_assert(RS_TV_OK == AKZ_BT_TV_OK && RS_TVC_OK == AKZ_BT_TVC_OK && RS_CV_NOT_RECORDED == AKZ_BT_NOT_RECORDED, "the stages' own verdicts");
static_assert(RS_JP_MAX_FEATURES * 2 * sizeof(uint32_t) <= 80 * 1024, "the two maps of a scene live in LDS");

struct JpCall {
    const uint32_t* pairs;        // [n_slots][cap][2]
    const uint32_t* npairs;       // [n_slots]
    const uint32_t* inliers;      // [n_slots][cap]
    const uint32_t* n_inliers;    // [n_slots]
    const uint32_t* best_id;      // [n_slots]
    const double* pose;           // [n_slots][12]
    const uint32_t* slots;        // [2][n_scenes] scratch: first, second
    uint32_t* plain;              // [n_scenes][cap][3] scratch: the triples in front of the shuffle
    uint32_t* triples;
    uint32_t* ntriples;
    uint32_t* first_only;
    uint32_t* nfirst;
    uint32_t* second_only;
    uint32_t* nsecond;
    double* pose_first;
    double* pose_second;
    uint32_t* verdict;
    unsigned long long seed;
    uint32_t cap, n_scenes, minimum, shuffle;
};

__global__ __launch_bounds__(kJpBlock) void k_jp_join(JpCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_cnt[2][kJpWaves];
    __shared__ uint32_t s_tot[256];
    uint32_t* map_f = reinterpret_cast<uint32_t*>(smem);
    uint32_t* map_s = map_f + a.cap;
    const uint32_t s = blockIdx.x, sa = a.slots[s], sb = a.slots[a.n_scenes + s];          // below n_slots: checked on the host
    const uint32_t *pa = a.pairs + 2 * (size_t)sa * a.cap, *pb = a.pairs + 2 * (size_t)sb * a.cap;
    const uint32_t *ia = a.inliers + (size_t)sa * a.cap, *ib = a.inliers + (size_t)sb * a.cap;
    if (threadIdx.x < 12u) a.pose_first[12 * (size_t)s + threadIdx.x] = a.pose[12 * (size_t)sa + threadIdx.x];
    else if (threadIdx.x < 24u) a.pose_second[12 * (size_t)s + threadIdx.x - 12u] = a.pose[12 * (size_t)sb + threadIdx.x - 12u];
    const uint32_t n1 = a.n_inliers[sa], n2 = a.n_inliers[sb], np1 = a.npairs[sa], np2 = a.npairs[sb];
    uint32_t v = akz_jp_counts_verdict(a.best_id[sa], a.best_id[sb], n1, n2, np1, np2, a.cap, a.minimum), c, o;
    if (v == (uint32_t)AKZ_JP_OK) {                                                      // uniform; n1, n2, np1, np2 <= cap
        bool bad = false;
        for (uint32_t i = threadIdx.x; i < n1; i += kJpBlock) bad = bad || !akz_jp_pair(pa, ia, i, np1, a.cap, &c, &o);
        for (uint32_t i = threadIdx.x; i < n2; i += kJpBlock) bad = bad || !akz_jp_pair(pb, ib, i, np2, a.cap, &c, &o);
        if (__syncthreads_or(bad)) v = AKZ_JP_BAD_INDEX;
    }
    if (v != (uint32_t)AKZ_JP_OK) {
        if (threadIdx.x == 0) {
            a.verdict[s] = v;
            a.ntriples[s] = 0u; a.nfirst[s] = 0u; a.nsecond[s] = 0u;
        }
        return;
    }
    for (uint32_t j = threadIdx.x; j < 2u * a.cap; j += kJpBlock) map_f[j] = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n1; i += kJpBlock) {
        akz_jp_pair(pa, ia, i, np1, a.cap, &c, &o);
        atomicMax(&map_f[c], akz_jp_map_word(i));                                        // c < cap
    }
    for (uint32_t i = threadIdx.x; i < n2; i += kJpBlock) {
        akz_jp_pair(pb, ib, i, np2, a.cap, &c, &o);
        atomicMax(&map_s[c], akz_jp_map_word(i));
    }
    __syncthreads();
    uint32_t* t = (a.shuffle ? a.plain : a.triples) + 3 * (size_t)s * a.cap;
    uint32_t *f = a.first_only + 2 * (size_t)s * a.cap, *g = a.second_only + 2 * (size_t)s * a.cap;
    uint32_t nt = 0u, nf = 0u, ns = 0u, tick = 0u, total;
    for (uint32_t i0 = 0; i0 < n1; i0 += kJpBlock) {                                     // ranks below n1 <= cap
        const uint32_t i = i0 + threadIdx.x;
        uint32_t at_s = 0u;
        if (i < n1) {
            akz_jp_pair(pa, ia, i, np1, a.cap, &c, &o);
            at_s = map_s[c];
        }
        const bool common = i < n1 && at_s != 0u, alone = i < n1 && at_s == 0u;
        uint32_t rank = akz_block_scan<kJpWaves>(s_cnt, tick, common, &total);
        if (common) {
            uint32_t c2, o2;
            akz_jp_pair(pb, ib, at_s - 1u, np2, a.cap, &c2, &o2);
            t[3 * (nt + rank)] = c; t[3 * (nt + rank) + 1] = o; t[3 * (nt + rank) + 2] = o2;
        }
        nt += total;
        rank = akz_block_scan<kJpWaves>(s_cnt, tick, alone, &total);
        if (alone) {
            f[2 * (nf + rank)] = c; f[2 * (nf + rank) + 1] = o;
        }
        nf += total;
    }
    for (uint32_t i0 = 0; i0 < n2; i0 += kJpBlock) {
        const uint32_t i = i0 + threadIdx.x;
        bool alone = false;
        if (i < n2) {
            akz_jp_pair(pb, ib, i, np2, a.cap, &c, &o);
            alone = map_f[c] == 0u;
        }
        const uint32_t rank = akz_block_scan<kJpWaves>(s_cnt, tick, alone, &total);
        if (alone) {
            g[2 * (ns + rank)] = c; g[2 * (ns + rank) + 1] = o;
        }
        ns += total;
    }
    if (threadIdx.x == 0) {
        a.verdict[s] = v;
        a.ntriples[s] = nt; a.nfirst[s] = nf; a.nsecond[s] = ns;
    }
    if (!a.shuffle) return;
    __syncthreads();                                                                     // the maps are read; the plain triples written
    uint32_t* rk = reinterpret_cast<uint32_t*>(smem);                                    // nt <= cap <= kRadixSortMax
    uint32_t* ia_ = rk + kRadixSortMax;
    uint32_t* ib_ = ia_ + kRadixSortMax;
    uint32_t* wh = ib_ + kRadixSortMax;
    const unsigned long long ss = akz_bt_scene_seed(a.seed, s);
    for (uint32_t j = threadIdx.x; j < nt; j += kJpBlock) {
        rk[j] = akz_bt_shuffle_key(ss, j);
        ia_[j] = j;
    }
    __syncthreads();
    const uint32_t* sorted = lds_radix_sort_ids(rk, ia_, ib_, wh, s_tot, nt, 4);
    uint32_t* out = a.triples + 3 * (size_t)s * a.cap;
    for (uint32_t j = threadIdx.x; j < nt; j += kJpBlock) {
        const uint32_t* src = t + 3 * (size_t)sorted[j];
        out[3 * j] = src[0]; out[3 * j + 1] = src[1]; out[3 * j + 2] = src[2];
    }
}

// words of ArCall::info
enum { kInfoBad = 0, kInfoRows = 1, kInfoTotal = 2, kInfoZero = 3, kInfoWords = 8 };
// words of a scene in ArCall::scene
enum { kScState = 0, kScTriples = 1, kScFirst = 2, kScSecond = 3, kScAccepted = 4, kScRow = 5, kScAt = 6, kScWords = 8 };
enum { kStateOff = 0, kStateValid = 1, kStateBad = 2 };

// everything the kernels of one call share, by value
struct ArCall {
    const uint32_t* triples; const uint32_t* ntriples; const uint32_t* first_only; const uint32_t* nfirst;
    const uint32_t* second_only; const uint32_t* nsecond;
    const unsigned char* combined; const unsigned char* first_ok; const unsigned char* second_ok;
    const double* pose_out;       // [n_scenes][2][12]
    const uint32_t* tv_verdict;   // [n_scenes]
    const uint32_t* kps;          // [n_src_blocks][cap] keypoints, as words
    const uint32_t* counts;       // [n_src_blocks]
    const uint32_t* skip;         // [n_scenes] or null
    const uint32_t* obs_start;    // [n_landmarks + 1] (a zero word of the scratch when there is no table)
    const uint2* obs;             // [n_obs]
    const uint32_t* recon_start;  // [n_recons + 1] or null
    const uint32_t* view_start;   // [n_recons + 1] or null
    uint32_t* kps_dst; uint32_t* counts_dst; double* poses;
    uint32_t* obs_start_out; uint2* obs_out; uint32_t* obs_counts_out; uint32_t* counts_out; uint32_t* landmarks_out;
    uint32_t* recon_start_out; uint32_t* view_start_out; uint32_t* views_out; double* constraint_poses_out;
    uint32_t* constraint_verdict_out; uint32_t* frame_verdict; uint32_t* stats; uint32_t* call_verdict;
    // scratch
    uint32_t* info;               // [kInfoWords]
    uint32_t* taken;              // [n_src_blocks]
    uint32_t* frames;             // [3][n_scenes] ic, i_first, i_second
    uint32_t* scene;              // [n_scenes][kScWords]
    uint32_t* maps;               // [n_scenes][5][cap] claimed centre features, their first / second feature, used first / second features
    uint32_t cap, n_scenes, n_src_blocks, n_obs, n_landmarks, n_recons, n_blocks, view_base, lm_room;
};

__global__ __launch_bounds__(kTblBlock) void k_bt_check_table(ArCall a)
{
    const uint32_t l = blockIdx.x * kTblBlock + threadIdx.x;
    int bad = l <= a.n_landmarks && akz_lt_start_bad(a.obs_start, l, a.n_landmarks, a.n_obs);
    if (a.n_recons && l <= a.n_recons)
        bad = bad || akz_ar_range_bad(a.recon_start, l, a.n_recons, a.n_landmarks) || akz_ar_range_bad(a.view_start, l, a.n_recons, a.view_base);
    tbl_flag(&a.info[kInfoBad], bad);
}

// observation {blk, feat} is written at obs_out[at] as a member of row `key`
__device__ __forceinline__ void bt_put(const ArCall& a, uint32_t at, uint32_t blk, uint32_t feat, uint32_t key)
{
    tbl_put(a.obs_out, a.landmarks_out, a.n_blocks, a.cap, at, make_uint2(blk, feat), key);
}

__global__ __launch_bounds__(kTblBlock) void k_bt_old(ArCall a)
{
    const uint32_t l = blockIdx.x * kTblBlock + threadIdx.x;
    const bool bad = a.info[kInfoBad] != 0u;
    if (l < a.n_landmarks) {
        a.obs_start_out[l] = a.obs_start[l];
        a.obs_counts_out[l] = akz_ar_old_length(a.obs_start, l);
        if (!bad)                                                        // the starts ascend inside [0, n_obs] <= obs_room
            for (uint32_t i = a.obs_start[l], e = a.obs_start[l + 1]; i < e; ++i) bt_put(a, i, a.obs[i].x, a.obs[i].y, l);
    }
    if (bad && l < a.n_obs) a.obs_out[l] = a.obs[l];
    if (l < a.n_recons) {
        a.recon_start_out[l] = a.recon_start[l];
        a.view_start_out[l] = a.view_start[l];
    }
}

// One workgroup per scene.  info and taken are zero in front of it.
__global__ __launch_bounds__(kTblBlock) void k_bt_validate(ArCall a)
{
    __shared__ uint32_t s_bad, s_n[3];
    const uint32_t s = blockIdx.x, bc = a.frames[s], bf = a.frames[a.n_scenes + s], bs = a.frames[2 * a.n_scenes + s];   // below n_src_blocks: the host
    const uint32_t cc = a.counts[bc], cf = a.counts[bf], cs = a.counts[bs], nt = a.ntriples[s], nf = a.nfirst[s], ns = a.nsecond[s];
    const bool off = a.info[kInfoBad] != 0u || a.tv_verdict[s] != (uint32_t)AKZ_BT_TV_OK || (a.skip && a.skip[s] != 0u);
    const bool counts_ok = akz_ar_counts_ok(bc, bf, bs, cc, cf, cs, nt, nf, ns, a.cap);
    uint32_t* cen = a.maps + 5 * (size_t)s * a.cap;
    uint32_t *cen_f = cen + a.cap, *cen_s = cen + 2 * (size_t)a.cap, *fst = cen + 3 * (size_t)a.cap, *snd = cen + 4 * (size_t)a.cap;
    for (uint32_t j = threadIdx.x; j < 5u * a.cap; j += kTblBlock) cen[j] = AKZ_LT_NONE;
    if (threadIdx.x < 3u) s_n[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    if (!off && counts_ok) {                                             // every count <= cap
        uint32_t bad = 0u, mt = 0u, mf = 0u, ms = 0u;
        const uint32_t *t = a.triples + 3 * (size_t)s * a.cap, *f = a.first_only + 2 * (size_t)s * a.cap, *g = a.second_only + 2 * (size_t)s * a.cap;
        for (uint32_t i = threadIdx.x; i < nt; i += kTblBlock) {
            if (!a.combined[(size_t)s * a.cap + i]) continue;
            const uint32_t c = t[3 * i], x = t[3 * i + 1], y = t[3 * i + 2];
            if (c >= cc || x >= cf || y >= cs) { bad = 1u; continue; }
            if (atomicCAS(&cen[c], AKZ_LT_NONE, 0u) != AKZ_LT_NONE) { bad = 1u; continue; }
            if (atomicCAS(&fst[x], AKZ_LT_NONE, c) != AKZ_LT_NONE || atomicCAS(&snd[y], AKZ_LT_NONE, c) != AKZ_LT_NONE) bad = 1u;
            cen_f[c] = x; cen_s[c] = y;                                  // the only claimant of c
            ++mt;
        }
        for (uint32_t i = threadIdx.x; i < nf; i += kTblBlock) {
            if (!a.first_ok[(size_t)s * a.cap + i]) continue;
            const uint32_t c = f[2 * i], x = f[2 * i + 1];
            if (c >= cc || x >= cf) { bad = 1u; continue; }
            if (atomicCAS(&cen[c], AKZ_LT_NONE, 0u) != AKZ_LT_NONE) { bad = 1u; continue; }
            if (atomicCAS(&fst[x], AKZ_LT_NONE, c) != AKZ_LT_NONE) bad = 1u;
            cen_f[c] = x;
            ++mf;
        }
        for (uint32_t i = threadIdx.x; i < ns; i += kTblBlock) {
            if (!a.second_ok[(size_t)s * a.cap + i]) continue;
            const uint32_t c = g[2 * i], y = g[2 * i + 1];
            if (c >= cc || y >= cs) { bad = 1u; continue; }
            if (atomicCAS(&cen[c], AKZ_LT_NONE, 0u) != AKZ_LT_NONE) { bad = 1u; continue; }
            if (atomicCAS(&snd[y], AKZ_LT_NONE, c) != AKZ_LT_NONE) bad = 1u;
            cen_s[c] = y;
            ++ms;
        }
        if (bad) atomicOr(&s_bad, 1u);
        if (mt) atomicAdd(&s_n[0], mt);
        if (mf) atomicAdd(&s_n[1], mf);
        if (ms) atomicAdd(&s_n[2], ms);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* sc = a.scene + (size_t)kScWords * s;
        sc[kScState] = off ? kStateOff : (counts_ok && s_bad == 0u) ? kStateValid : kStateBad;
        sc[kScTriples] = s_n[0]; sc[kScFirst] = s_n[1]; sc[kScSecond] = s_n[2];
    }
}

// ONE lane: acceptance in scene order and everything that follows from it alone
__global__ void k_bt_accept(ArCall a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool bad = a.info[kInfoBad] != 0u;
    const uint32_t old_rows = a.n_recons ? a.recon_start[a.n_recons] : a.n_landmarks, old_views = a.n_recons ? a.view_start[a.n_recons] : a.view_base;
    uint32_t row = a.n_landmarks, at = a.obs_start[a.n_landmarks], accepted_n = 0u;
    for (uint32_t s = 0; s < a.n_scenes; ++s) {
        uint32_t* sc = a.scene + (size_t)kScWords * s;
        const uint32_t bc = a.frames[s], bf = a.frames[a.n_scenes + s], bs = a.frames[2 * a.n_scenes + s];
        uint32_t v = sc[kScState] == kStateOff ? AKZ_AR_NOT_ACCEPTED : sc[kScState] == kStateBad ? AKZ_AR_BAD_INDEX : AKZ_AR_OK;
        if (v == (uint32_t)AKZ_AR_OK && (a.taken[bc] || a.taken[bf] || a.taken[bs])) v = AKZ_AR_TAKEN;
        const bool ok = v == (uint32_t)AKZ_AR_OK;
        a.frame_verdict[s] = v;
        a.recon_start_out[a.n_recons + s] = bad ? old_rows : row;
        a.view_start_out[a.n_recons + s] = bad ? old_views : akz_ar_view(a.view_base, s, 0);
        for (uint32_t k = 0; k < 3u; ++k) a.views_out[3 * (size_t)s + k] = akz_ar_view(a.view_base, s, k);
        a.constraint_verdict_out[s] = ok ? (uint32_t)AKZ_BT_TVC_OK : (uint32_t)AKZ_BT_NOT_RECORDED;
        sc[kScAccepted] = ok ? 1u : 0u;
        sc[kScRow] = row;
        sc[kScAt] = at;
        uint32_t* st = a.stats + (size_t)AKZ_AR_STATS * s;
        const uint32_t mt = sc[kScTriples], mf = sc[kScFirst], ms = sc[kScSecond];
        const uint32_t cc = a.counts[bc], cf = a.counts[bf], cs = a.counts[bs];
        const uint32_t rows = ok ? akz_ar_scene_rows(cc, cf, cs, mt + mf, mt + ms) : 0u;
        st[AKZ_AR_S_TRIPLES] = ok ? mt : 0u; st[AKZ_AR_S_FIRST] = ok ? mf : 0u; st[AKZ_AR_S_SECOND] = ok ? ms : 0u;
        st[AKZ_AR_S_LANDMARKS] = rows;
        if (!ok) continue;
        a.taken[bc] = 1u; a.taken[bf] = 1u; a.taken[bs] = 1u;
        ++accepted_n;
        row += rows;                                                     // <= n_landmarks + 3 n_scenes cap <= lm_room
        at += cc + cf + cs;                                              // every feature of the three views is observed once
    }
    const uint32_t rows = bad ? a.n_landmarks : row, total = bad ? a.obs_start[a.n_landmarks] : at;
    a.recon_start_out[a.n_recons + a.n_scenes] = bad ? old_rows : rows;
    a.view_start_out[a.n_recons + a.n_scenes] = bad ? old_views : akz_ar_view(a.view_base, a.n_scenes, 0);
    a.info[kInfoRows] = rows;
    a.info[kInfoTotal] = total;
    a.counts_out[AKZ_AR_C_ROWS] = rows;
    a.counts_out[AKZ_AR_C_OBSERVATIONS] = bad ? a.n_obs : total;
    a.counts_out[AKZ_AR_C_RECONSTRUCTIONS] = a.n_recons + a.n_scenes;
    a.counts_out[AKZ_AR_C_ACCEPTED] = accepted_n;
    *a.call_verdict = bad ? AKZ_AR_BAD_TABLE : AKZ_AR_OK;
}

// grid (words of a block / kTblBlock, 3, scenes)
__global__ __launch_bounds__(kTblBlock) void k_bt_copy(ArCall a)
{
    const uint32_t s = blockIdx.z, k = blockIdx.y, w = blockIdx.x * kTblBlock + threadIdx.x;
    if (!a.scene[(size_t)kScWords * s + kScAccepted]) return;
    const uint32_t src = a.frames[k * a.n_scenes + s], view = akz_ar_view(a.view_base, s, k);       // view < n_blocks: the host
    const size_t words = (size_t)a.cap * kKpWords;
    if (w < words) a.kps_dst[view * words + w] = a.kps[src * words + w];
    if (w == 0u) a.counts_dst[view] = a.counts[src];
    if (w < 12u) a.poses[12 * (size_t)view + w] = k == 0u ? ((w == 0u || w == 5u || w == 10u) ? 1.0 : 0.0) : a.pose_out[24 * (size_t)s + 12 * (k - 1u) + w];
    if (k == 0u && w < 24u) a.constraint_poses_out[24 * (size_t)s + w] = a.pose_out[24 * (size_t)s + w];
}

// grid (tiles of a block's features, scenes)
__global__ __launch_bounds__(kTblBlock) void k_bt_rows(ArCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t s = blockIdx.y, first = blockIdx.x * kTblTile;
    const uint32_t* sc = a.scene + (size_t)kScWords * s;
    if (!sc[kScAccepted]) return;
    const uint32_t cc = a.counts[a.frames[s]];                            // <= cap: the scene is valid
    if (first >= cc) return;
    const uint32_t* cen_f = a.maps + (5 * (size_t)s + 1) * a.cap;
    const uint32_t* cen_s = cen_f + a.cap;
    uint32_t before = 0u, tick = 0u;
    for (uint32_t j = threadIdx.x; j < first; j += kTblBlock) before += akz_ar_row_length(cen_f[j], cen_s[j]);
    uint32_t run = sc[kScAt] + akz_block_sum<kTblWaves>(s_cnt, tick, before);
#pragma unroll 1
    for (int it = 0; it < kTblItems; ++it) {
        const uint32_t j = first + (uint32_t)it * kTblBlock + threadIdx.x;
        const bool on = j < cc;
        const uint32_t x = on ? cen_f[j] : AKZ_LT_NONE, y = on ? cen_s[j] : AKZ_LT_NONE, len = on ? akz_ar_row_length(x, y) : 0u;
        uint32_t dst = tbl_scan_step(run, len, s_wave);
        if (!on) continue;
        const uint32_t r = sc[kScRow] + j;
        a.obs_start_out[r] = dst;
        a.obs_counts_out[r] = len;
        bt_put(a, dst++, akz_ar_view(a.view_base, s, 0), j, r);           // dst + len <= n_obs + 3 n_scenes cap <= obs_room
        if (x != AKZ_LT_NONE) bt_put(a, dst++, akz_ar_view(a.view_base, s, 1), x, r);
        if (y != AKZ_LT_NONE) bt_put(a, dst++, akz_ar_view(a.view_base, s, 2), y, r);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_bt_new_rows(ArCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    const uint32_t s = blockIdx.x;
    const uint32_t* sc = a.scene + (size_t)kScWords * s;
    if (!sc[kScAccepted]) return;
    const uint32_t cc = a.counts[a.frames[s]], mt = sc[kScTriples];
    uint32_t row = sc[kScRow] + cc, at = sc[kScAt] + akz_ar_centre_observations(cc, mt + sc[kScFirst], mt + sc[kScSecond]), tick = 0u;
    for (uint32_t k = 1; k < 3u; ++k) {
        const uint32_t count = a.counts[a.frames[k * a.n_scenes + s]];    // <= cap
        const uint32_t* used = a.maps + (5 * (size_t)s + 2 + k) * a.cap;
        for (uint32_t j0 = 0; j0 < count; j0 += kTblBlock) {
            const uint32_t j = j0 + threadIdx.x;
            const bool fresh = j < count && used[j] == AKZ_LT_NONE;
            uint32_t total;
            const uint32_t rank = akz_block_scan<kTblWaves>(s_cnt, tick, fresh, &total);
            if (fresh) {
                a.obs_start_out[row + rank] = at + rank;
                a.obs_counts_out[row + rank] = 1u;
                bt_put(a, at + rank, akz_ar_view(a.view_base, s, k), j, row + rank);
            }
            row += total;
            at += total;
        }
    }
}

}   // namespace

extern "C" int32_t rs_join_pairs_batch_device(rs_ctx* c, const void* d_pairs, const void* d_npairs, const void* d_inliers, const void* d_n_inliers,
                                              const void* d_best_id, const void* d_pose, uint32_t n_slots, uint32_t cap_per_img,
                                              const uint32_t* slot_first, const uint32_t* slot_second, uint32_t n_scenes,
                                              uint32_t two_view_minimum_robust_matches, uint32_t flags, uint64_t seed, void* d_triples,
                                              void* d_ntriples, void* d_first_only, void* d_nfirst, void* d_second_only, void* d_nsecond,
                                              void* d_pose_first, void* d_pose_second, void* d_verdict, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (cap_per_img == 0 || n_scenes > 65535u || (flags & ~(uint32_t)RS_BATCH_SHUFFLE)) return AKZ_E_INVALID;
        const bool shuffle = (flags & RS_BATCH_SHUFFLE) != 0;
        if (cap_per_img > (uint32_t)RS_JP_MAX_FEATURES || (shuffle && cap_per_img > kRadixSortMax)) return AKZ_E_TOO_LARGE;
        if (n_scenes != 0 && (!d_pairs || !d_npairs || !d_inliers || !d_n_inliers || !d_best_id || !d_pose || !slot_first || !slot_second ||
                              !d_triples || !d_ntriples || !d_first_only || !d_nfirst || !d_second_only || !d_nsecond || !d_pose_first ||
                              !d_pose_second || !d_verdict))
            return AKZ_E_INVALID;
        for (uint32_t s = 0; s < n_scenes; ++s)
            if (slot_first[s] >= n_slots || slot_second[s] >= n_slots) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        if (n_scenes == 0) return AKZ_OK;
        const size_t w = sizeof(uint32_t), slot_bytes = akz_align_up(w * 2 * (size_t)n_scenes, 256);
        const size_t plain_bytes = shuffle ? w * 3 * (size_t)n_scenes * cap_per_img : 0;
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, slot_bytes + plain_bytes));
        char* base = (char*)ls->d_scratch;
        AKZ_HIP(hipMemcpyAsync(base, slot_first, w * n_scenes, hipMemcpyHostToDevice, h.stream));
        AKZ_HIP(hipMemcpyAsync(base + w * n_scenes, slot_second, w * n_scenes, hipMemcpyHostToDevice, h.stream));
        JpCall a;
        a.pairs = (const uint32_t*)d_pairs; a.npairs = (const uint32_t*)d_npairs; a.inliers = (const uint32_t*)d_inliers;
        a.n_inliers = (const uint32_t*)d_n_inliers; a.best_id = (const uint32_t*)d_best_id; a.pose = (const double*)d_pose;
        a.slots = (const uint32_t*)base; a.plain = (uint32_t*)(base + slot_bytes);
        a.triples = (uint32_t*)d_triples; a.ntriples = (uint32_t*)d_ntriples; a.first_only = (uint32_t*)d_first_only; a.nfirst = (uint32_t*)d_nfirst;
        a.second_only = (uint32_t*)d_second_only; a.nsecond = (uint32_t*)d_nsecond; a.pose_first = (double*)d_pose_first;
        a.pose_second = (double*)d_pose_second; a.verdict = (uint32_t*)d_verdict;
        a.seed = (unsigned long long)seed; a.cap = cap_per_img; a.n_scenes = n_scenes; a.minimum = two_view_minimum_robust_matches;
        a.shuffle = shuffle ? 1u : 0u;
        size_t lds = w * 2 * (size_t)cap_per_img;
        if (shuffle && lds < kRadixSortLdsBytes) lds = kRadixSortLdsBytes;
        if (lds > 32768) AKZ_HIP(hipFuncSetAttribute((const void*)k_jp_join, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_jp_join, dim3(n_scenes), dim3(kJpBlock), lds, h.stream, a);
        AKZ_LAUNCH_CHECK();
        // the slot lists are pageable host memory: the copies above have returned, the caller may free them
        return AKZ_OK;
    });
}

extern "C" int32_t rs_add_reconstruction_batch_device(
    rs_ctx* c, const void* d_triples, const void* d_ntriples, const void* d_first_only, const void* d_nfirst, const void* d_second_only,
    const void* d_nsecond, const void* d_combined, const void* d_first_ok, const void* d_second_ok, const void* d_pose_out, const void* d_verdict,
    const uint32_t* ic, const uint32_t* i_first, const uint32_t* i_second, uint32_t n_scenes, const void* d_kps, const void* d_counts,
    uint32_t n_src_blocks, uint32_t cap_per_img, const void* d_skip, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
    uint32_t n_landmarks, const void* d_recon_start, const void* d_view_start, uint32_t n_recons, void* d_kps_dst, void* d_counts_dst,
    void* d_poses, uint32_t n_blocks, uint32_t view_base, uint32_t obs_room, uint32_t lm_room, void* d_obs_start_out, void* d_obs_out,
    void* d_obs_counts_out, void* d_counts_out, void* d_landmarks_out, void* d_recon_start_out, void* d_view_start_out, void* d_views_out,
    void* d_constraint_poses_out, void* d_constraint_verdict_out, void* d_frame_verdict, void* d_stats, void* d_call_verdict,
    void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_obs_start_out || !d_obs_out || !d_obs_counts_out || !d_counts_out || !d_landmarks_out || !d_recon_start_out || !d_view_start_out ||
            !d_call_verdict)
            return AKZ_E_INVALID;
        if (n_scenes != 0 && (!d_triples || !d_ntriples || !d_first_only || !d_nfirst || !d_second_only || !d_nsecond || !d_combined ||
                              !d_first_ok || !d_second_ok || !d_pose_out || !d_verdict || !ic || !i_first || !i_second || !d_kps || !d_counts ||
                              !d_kps_dst || !d_counts_dst || !d_poses || !d_views_out || !d_constraint_poses_out || !d_constraint_verdict_out ||
                              !d_frame_verdict || !d_stats))
            return AKZ_E_INVALID;
        if ((n_landmarks != 0 && !d_obs_start) || (n_obs != 0 && !d_obs) || (!d_obs_start && n_obs != 0)) return AKZ_E_INVALID;
        if ((n_recons != 0) != (d_recon_start != nullptr) || (n_recons != 0) != (d_view_start != nullptr)) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || n_scenes > 65535u || n_recons > 0xFFFFFFFFu - 65536u) return AKZ_E_INVALID;
        // row numbers of the last tile and the words of a keypoint block stay 32-bit
        if (n_landmarks > 0xFFFFFFFFu - 2u * kTblTile || cap_per_img > kAkzMaxKeypoints) return AKZ_E_TOO_LARGE;
        if ((uint64_t)view_base + 3ull * n_scenes > (uint64_t)n_blocks) return AKZ_E_INVALID;
        // the rooms: no kernel can write past them (every feature of a scene's views adds one observation and at most one row)
        const uint64_t grow = 3ull * n_scenes * cap_per_img;
        if ((uint64_t)obs_room < (uint64_t)n_obs + grow || (uint64_t)lm_room < (uint64_t)n_landmarks + grow || lm_room == 0xFFFFFFFFu)
            return AKZ_E_INVALID;
        for (uint32_t s = 0; s < n_scenes; ++s)
            if (ic[s] >= n_src_blocks || i_first[s] >= n_src_blocks || i_second[s] >= n_src_blocks) return AKZ_E_INVALID;
        // the keypoint pools: apart, or one pool whose destination range holds no source block of the call
        const size_t block_bytes = sizeof(akz_keypoint) * (size_t)cap_per_img;
        if (n_scenes) {
            if (d_kps_dst == d_kps) {
                for (uint32_t s = 0; s < n_scenes; ++s)
                    for (uint32_t b : {ic[s], i_first[s], i_second[s]})
                        if (b >= view_base && b < view_base + 3u * n_scenes) return AKZ_E_INVALID;
            } else if (akz_ranges_overlap(d_kps, block_bytes * n_src_blocks, d_kps_dst, block_bytes * n_blocks)) {
                return AKZ_E_INVALID;
            }
        }
        // the input table is const: no output table may lie over it
        const size_t w = sizeof(uint32_t);
        const void* in[4] = {d_obs_start, d_obs, d_recon_start, d_view_start};
        const size_t in_bytes[4] = {w * ((size_t)n_landmarks + 1), w * 2 * (size_t)n_obs, w * ((size_t)n_recons + 1), w * ((size_t)n_recons + 1)};
        const void* out[7] = {d_obs_start_out, d_obs_out, d_obs_counts_out, d_landmarks_out, d_counts_out, d_recon_start_out, d_view_start_out};
        const size_t range_bytes = w * ((size_t)n_recons + n_scenes + 1);
        const size_t out_bytes[7] = {w * ((size_t)lm_room + 1), w * 2 * (size_t)obs_room, w * (size_t)lm_room, w * (size_t)n_blocks * cap_per_img,
                                     w * AKZ_AR_COUNTS, range_bytes, range_bytes};
        if (!akz_outputs_clear_of_inputs(in, in_bytes, 4, out, out_bytes, 7)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        AkzScratchPlan plan;                                             // zero: info, taken
        const size_t at_info = plan.take(w * kInfoWords), at_taken = plan.take(w * ((size_t)n_src_blocks + 1)), at_frames = plan.take(w * (3 * (size_t)n_scenes + 1));
        const size_t at_scene = plan.take(w * (kScWords * (size_t)n_scenes + 1)), at_maps = plan.take(w * (5 * (size_t)n_scenes * cap_per_img + 1));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, plan.size()));
        char* base = (char*)ls->d_scratch;
        ArCall a;
        a.info = (uint32_t*)(base + at_info); a.taken = (uint32_t*)(base + at_taken); a.frames = (uint32_t*)(base + at_frames);
        a.scene = (uint32_t*)(base + at_scene); a.maps = (uint32_t*)(base + at_maps);
        a.triples = (const uint32_t*)d_triples; a.ntriples = (const uint32_t*)d_ntriples; a.first_only = (const uint32_t*)d_first_only;
        a.nfirst = (const uint32_t*)d_nfirst; a.second_only = (const uint32_t*)d_second_only; a.nsecond = (const uint32_t*)d_nsecond;
        a.combined = (const unsigned char*)d_combined; a.first_ok = (const unsigned char*)d_first_ok; a.second_ok = (const unsigned char*)d_second_ok;
        a.pose_out = (const double*)d_pose_out; a.tv_verdict = (const uint32_t*)d_verdict; a.kps = (const uint32_t*)d_kps;
        a.counts = (const uint32_t*)d_counts; a.skip = (const uint32_t*)d_skip;
        a.obs_start = d_obs_start ? (const uint32_t*)d_obs_start : a.info + kInfoZero;      // no table: one start, 0
        a.obs = (const uint2*)d_obs; a.recon_start = (const uint32_t*)d_recon_start; a.view_start = (const uint32_t*)d_view_start;
        a.kps_dst = (uint32_t*)d_kps_dst; a.counts_dst = (uint32_t*)d_counts_dst; a.poses = (double*)d_poses;
        a.obs_start_out = (uint32_t*)d_obs_start_out; a.obs_out = (uint2*)d_obs_out; a.obs_counts_out = (uint32_t*)d_obs_counts_out;
        a.counts_out = (uint32_t*)d_counts_out; a.landmarks_out = (uint32_t*)d_landmarks_out; a.recon_start_out = (uint32_t*)d_recon_start_out;
        a.view_start_out = (uint32_t*)d_view_start_out; a.views_out = (uint32_t*)d_views_out; a.constraint_poses_out = (double*)d_constraint_poses_out;
        a.constraint_verdict_out = (uint32_t*)d_constraint_verdict_out; a.frame_verdict = (uint32_t*)d_frame_verdict; a.stats = (uint32_t*)d_stats;
        a.call_verdict = (uint32_t*)d_call_verdict;
        a.cap = cap_per_img; a.n_scenes = n_scenes; a.n_src_blocks = n_src_blocks; a.n_obs = n_obs; a.n_landmarks = n_landmarks;
        a.n_recons = n_recons; a.n_blocks = n_blocks; a.view_base = view_base; a.lm_room = lm_room;
        AKZ_HIP(hipMemsetAsync(base + at_info, 0, at_frames - at_info, h.stream));
        AKZ_HIP(hipMemsetAsync(d_landmarks_out, 0xFF, out_bytes[3], h.stream));
        if (n_scenes) {
            AKZ_HIP(hipMemcpyAsync(a.frames, ic, w * n_scenes, hipMemcpyHostToDevice, h.stream));
            AKZ_HIP(hipMemcpyAsync(a.frames + n_scenes, i_first, w * n_scenes, hipMemcpyHostToDevice, h.stream));
            AKZ_HIP(hipMemcpyAsync(a.frames + 2 * (size_t)n_scenes, i_second, w * n_scenes, hipMemcpyHostToDevice, h.stream));
        }
        const dim3 block(kTblBlock);
        const uint32_t widest = n_landmarks > n_recons ? n_landmarks : n_recons, longest = widest > n_obs ? widest : n_obs;
        hipLaunchKernelGGL(k_bt_check_table, dim3(widest / kTblBlock + 1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_bt_old, dim3(longest / kTblBlock + 1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_scenes) {
            hipLaunchKernelGGL(k_bt_validate, dim3(n_scenes), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_bt_accept, dim3(1), dim3(64), 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_scenes) {
            const uint32_t words = cap_per_img * kKpWords;                                // cap_per_img <= kAkzMaxKeypoints
            hipLaunchKernelGGL(k_bt_copy, dim3((words + kTblBlock - 1) / kTblBlock, 3, n_scenes), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_bt_rows, dim3((cap_per_img + kTblTile - 1) / kTblTile, n_scenes), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_bt_new_rows, dim3(n_scenes), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_tbl_tail, dim3((lm_room - n_landmarks) / kTblBlock + 1), block, 0, h.stream, a.obs_start_out, a.obs_counts_out, n_landmarks,
                           lm_room, (const uint32_t*)&a.info[kInfoRows], (const uint32_t*)&a.info[kInfoTotal]);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
