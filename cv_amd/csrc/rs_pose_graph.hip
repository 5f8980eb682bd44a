// rs_pose_graph.hip — the relaxation of cv-sfm's pose graph under its three-view constraints on gfx950: what
// VSlam::apply_constraints does (cv-sfm/src/lib.rs:2358-2375) for n_graphs reconstructions side by side, optimization_iterations
// Jacobi rounds of constrain_view (lib.rs:1892-1936) over every view.  ONE WAVEFRONT PER VIEW AND ROUND, in every form:
//   k_pg_edges            one lane per constraint: its six expected other-to-target isometries (lib.rs:167-180).
//   k_pg_prepare          one workgroup per graph: every index of the graph is looked at before anything is read through one,
//                         the views' states, the counts, the verdicts that fall before round 0, and which form runs the graph.
//   k_pg_relax_resident   one persistent workgroup per graph of at most RS_PG_RESIDENT_VIEWS views (by default it is given the
//                         graphs of at most RS_PG_DEFAULT_RESIDENT_VIEWS = its 8 waves, see below): both pose tables in LDS
//                         (2 x 96 B per view, 48 KB), its waves loop over the views, a lane reads its edges' `expected` from
//                         global memory (constant over the rounds: L2 serves them) and world_to_other from the table of the
//                         round before, lane 0 writes the new pose into the other table; ONE workgroup barrier per round.
//   k_pg_relax_sweep      larger graphs: one launch per round over all views, one wave per view, the tables ping-pong between
//                         d_poses and the context's scratch; a graph that stopped says so in a device word that later rounds'
//                         waves read first.  No host synchronisation between rounds, no grid-wide barrier, no cooperative
//                         launch: the order of the rounds is the order of the launches on the stream.
//   k_pg_finish           the swept graphs' verdicts and stats, and the copy back when the last round landed in the scratch.
// The two forms give equal bits: a view's sum is one wave's, in the order include/akz_pose_graph_math.h fixes, whichever
// kernel the wave belongs to.  Every loop is bounded by a parameter or a validated range; nothing waits on another workgroup.
//
// Which form: measured on the MI355X (tools/bench_pose_graph.py), one view's round is a chain of FP64 latency of
// about 5 us (two products, a log map with its acos, the butterfly, an exponential map, a product), which the 8 waves of the
// resident workgroup repeat for their views one after another — 9.7 us a round at 16 views, 123 us at 256 —, while a launch
// per round costs 7 us whatever the number of views, up to the tens of thousands that fill the device.  The resident form is
// the faster one up to a wave per view, so that is what it takes unless rs_pose_graph_debug_resident_views says otherwise.
// The two forms of one call run one after the other on the stream and the host cannot know whether a graph needs the sweep,
// so in a call of more views than the limit the sweep's launches are enqueued whatever the graphs' sizes, and a resident
// kernel in front of them adds its time to theirs.  With a limit of at most a wave per view that can only lose: such a call
// is swept as a whole.  By default the resident kernel therefore serves calls of at most 8 views in all — one tiny graph, or
// two — and stands by for a caller who knows the graphs to be few and small enough to set a higher limit.
//
// The LDS tables are read one pose (12 consecutive doubles) per lane at 64 unrelated views: whatever the layout, such a
// gather conflicts in the banks; a round is bound by the latency of its log maps, not by these reads.
//
// The arithmetic is include/akz_pose_graph_math.h, the text the CPU checker (tests/cpp/pose_graph_host.c) compiles too —
// parity: host build == HIP, bit for bit.
#include "akz_common.h"
#include "../../include/akz_pose_graph_math.h"

#ifndef RS_PG_RESIDENT_WAVES
#define RS_PG_RESIDENT_WAVES 8    // waves of the persistent workgroup: 8 views of a graph move at once, two waves per SIMD.  A
                                  // view's round takes 162 VGPRs; 16 waves would hold it to 128 and spill 34 to scratch
#endif

namespace {

constexpr int kPgWave = AKZ_PG_WAVE;
static_assert(AKZ_PG_WAVE == 64, "akz_wave_sum adds over 64 lanes");
constexpr int kPgWaves = 4;                                   // of k_pg_prepare, k_pg_relax_sweep and k_pg_finish
constexpr int kPgBlock = kPgWave * kPgWaves;
constexpr int kPgResidentBlock = kPgWave * RS_PG_RESIDENT_WAVES;
constexpr uint32_t kPgNone = AKZ_PG_NO_VIEW;
enum : uint32_t { kPgDone = 0, kPgResident = 1, kPgSweep = 2 };   // d_form[g]: who runs graph g after k_pg_prepare

static_assert(RS_PG_OK == AKZ_PG_OK && RS_PG_FEW_VIEWS == AKZ_PG_FEW_VIEWS && RS_PG_NONFINITE == AKZ_PG_NONFINITE &&
              RS_PG_BAD_INDEX == AKZ_PG_BAD_INDEX, "verdict values");
static_assert(RS_PG_VIEW_UPDATED == AKZ_PG_VIEW_UPDATED && RS_PG_VIEW_NO_CONSTRAINT == AKZ_PG_VIEW_NO_CONSTRAINT &&
              RS_PG_VIEW_NONFINITE == AKZ_PG_VIEW_NONFINITE, "view states");
static_assert(RS_PG_STATS == AKZ_PG_STATS && RS_PG_S_VIEWS == AKZ_PG_S_VIEWS && RS_PG_S_UPDATED == AKZ_PG_S_UPDATED &&
              RS_PG_S_EDGES == AKZ_PG_S_EDGES && RS_PG_S_ROUNDS == AKZ_PG_S_ROUNDS && RS_PG_S_STAGE == AKZ_PG_S_STAGE &&
              RS_PG_S_FIRST_BAD_VIEW == AKZ_PG_S_FIRST_BAD_VIEW, "stats words");
static_assert(RS_PG_RESIDENT_VIEWS == AKZ_PG_RESIDENT_VIEWS && RS_PG_MAX_ITERATIONS == AKZ_PG_MAX_ITERATIONS, "limits");
static_assert(RS_PG_DEFAULT_RESIDENT_VIEWS == RS_PG_RESIDENT_WAVES, "by default the resident form takes the graphs it gives a wave per view");
static_assert(sizeof(double) * 2 * 12 * RS_PG_RESIDENT_VIEWS + 4 * RS_PG_RESIDENT_VIEWS + 64 <= 65536, "static LDS");

// everything a call's kernels share, by value
struct PgCall {
    double* poses;               // [n_views][12] the caller's table
    double* table;               // [n_views][12] the context's
    const uint32_t* graph_start; // [n_graphs + 1]
    const uint32_t* row_start;   // [n_views + 1]
    const uint32_t* row_edges;   // [n_rows]
    const uint32_t* views;       // [n_constraints][3]
    const uint32_t* cverdict;    // [n_constraints]
    const double* edges;         // [n_constraints][6][12]
    uint32_t* graph_verdict;     // [n_graphs]
    uint32_t* view_state;        // [n_views]
    uint32_t* stats;             // [n_graphs][AKZ_PG_STATS]
    uint32_t* view_graph;        // [n_views] scratch: the swept graph a view belongs to, kPgNone for every other view
    uint32_t* form;              // [n_graphs] scratch
    uint32_t* stop;              // [n_graphs] scratch: the round a swept graph stopped in, kPgNone while it runs
    const uint32_t* skip;        // [n_graphs] or null: nonzero = the graph is not run and none of its outputs is written
    uint32_t n_views, n_graphs, n_rows, n_constraints, iterations, resident_views;
    double rate;
};

__global__ __launch_bounds__(kPgBlock) void k_pg_edges(const double* __restrict__ cposes, const uint32_t* __restrict__ cverdict,
                                                       uint32_t n_constraints, double* __restrict__ edges)
{
    const uint32_t c = blockIdx.x * kPgBlock + threadIdx.x;
    if (c >= n_constraints) return;
    double e[72];
    if (cverdict[c] == (uint32_t)AKZ_TVC_OK) {
        double p[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) p[k] = cposes[(size_t)24 * c + k];
        akz_pg_constraint_edges(p, e);
    } else {
#pragma unroll
        for (int k = 0; k < 72; ++k) e[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 72; ++k) edges[(size_t)72 * c + k] = e[k];
}

// One workgroup per graph.  view_graph[v] carries a view's count of edges from the first pass to the second.
__global__ __launch_bounds__(kPgBlock) void k_pg_prepare(PgCall a)
{
    __shared__ uint32_t s_bad, s_updated, s_edges, s_before;
    const uint32_t g = blockIdx.x, lane = threadIdx.x & (kPgWave - 1), w = threadIdx.x / kPgWave;
    if (a.skip && a.skip[g] != 0u) {                  // (rs_internal_pose_graph_relax) the whole workgroup leaves together
        if (threadIdx.x == 0) { a.form[g] = kPgDone; a.stop[g] = kPgNone; }
        return;
    }
    if (threadIdx.x == 0) { s_bad = 0u; s_updated = 0u; s_edges = 0u; s_before = 0u; }
    __syncthreads();
    const uint32_t gs = a.graph_start[g], ge = a.graph_start[g + 1];
    // graph_start ascends up to this graph: no start before it lies above its own.  Two graphs that pass this and gs <= ge
    // cannot overlap, so a start array that runs backwards somewhere never lets two workgroups meet on a view.
    {
        uint32_t before = 0u;
        for (uint32_t k = threadIdx.x; k < g; k += kPgBlock) before = max(before, a.graph_start[k]);
        if (before > gs) atomicMax(&s_before, before);
    }
    __syncthreads();
    const bool range_ok = s_before <= gs && gs <= ge && ge <= a.n_views;
    if (range_ok)
        for (uint32_t v = gs + w; v < ge; v += kPgWaves) {
            const uint32_t rs = a.row_start[v], re = a.row_start[v + 1];
            int bad = rs > re || re > a.n_rows;
            uint32_t has = 0u, other;
            if (!bad)
                for (uint32_t i = rs + lane; i < re; i += kPgWave) {
                    const int r = akz_pg_entry(a.row_edges[i], v, gs, ge, a.views, a.cverdict, a.n_constraints, &other);
                    bad |= r < 0;
                    has += r > 0 ? 1u : 0u;
                }
            has = akz_wave_sum(has);
            bad = __any(bad);
            if (lane == 0) {
                a.view_graph[v] = has;
                if (bad) atomicOr(&s_bad, 1u);
                else if (has) { atomicAdd(&s_updated, 1u); atomicAdd(&s_edges, has); }
            }
        }
    __syncthreads();
    const bool ok = range_ok && s_bad == 0u;
    const uint32_t n = ok ? ge - gs : 0u, updated = s_updated;
    uint32_t form = kPgDone;
    if (ok && updated >= 3u && a.iterations != 0u) form = n <= a.resident_views ? kPgResident : kPgSweep;
    if (range_ok && lane == 0)
        for (uint32_t v = gs + w; v < ge; v += kPgWaves) {
            if (ok) a.view_state[v] = a.view_graph[v] ? AKZ_PG_VIEW_UPDATED : AKZ_PG_VIEW_NO_CONSTRAINT;
            a.view_graph[v] = form == kPgSweep ? g : kPgNone;
        }
    if (threadIdx.x == 0) {
        uint32_t* stats = a.stats + (size_t)AKZ_PG_STATS * g;
#pragma unroll
        for (int k = 0; k < AKZ_PG_STATS; ++k) stats[k] = 0u;
        stats[AKZ_PG_S_FIRST_BAD_VIEW] = kPgNone;
        if (ok) {
            stats[AKZ_PG_S_VIEWS] = n;
            stats[AKZ_PG_S_UPDATED] = updated;
            stats[AKZ_PG_S_EDGES] = s_edges;
            stats[AKZ_PG_S_STAGE] = updated < 3u ? AKZ_PG_STAGE_VIEWS : AKZ_PG_STAGE_ROUNDS;
        }
        a.graph_verdict[g] = !ok ? AKZ_PG_BAD_INDEX : updated < 3u ? AKZ_PG_FEW_VIEWS : AKZ_PG_OK;
        a.form[g] = form;
        a.stop[g] = kPgNone;
    }
}

// One view's round by one wave: src the table of the round before and dst the other one, both indexed by view - base (LDS:
// base = the graph's first view; global: 0).  Every index was looked at by k_pg_prepare.  -> 0: the net was not finite
// (dst = src for this view).
__device__ __forceinline__ int pg_view_round(const PgCall& a, const double* src, double* dst, uint32_t base, uint32_t v, uint32_t lane)
{
    double cur[12], inv[12], part[6], out[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) cur[k] = src[(size_t)12 * (v - base) + k];
    akz_tv_pose_inverse(cur, inv);
#pragma unroll
    for (int k = 0; k < 6; ++k) part[k] = 0.0;
    const uint32_t rs = a.row_start[v], re = a.row_start[v + 1];
    for (uint32_t i = rs + lane; i < re; i += kPgWave) {
        const uint32_t e = a.row_edges[i], c = e / 6u;
        if (a.cverdict[c] != (uint32_t)AKZ_TVC_OK) continue;          // + 0.0
        const uint32_t o = a.views[3 * (size_t)c + akz_pg_slot_other(e % 6u)];
        double ex[12], wo[12], q[6];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            ex[k] = a.edges[(size_t)12 * e + k];
            wo[k] = src[(size_t)12 * (o - base) + k];
        }
        akz_pg_edge_se3(ex, wo, inv, q);
#pragma unroll
        for (int k = 0; k < 6; ++k) part[k] = part[k] + q[k];
    }
    akz_wave_sum(part);
    const int ok = akz_pg_view_update(part, a.rate, cur, out);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) dst[(size_t)12 * (v - base) + k] = out[k];
    }
    return ok;
}

__global__ __launch_bounds__(kPgResidentBlock) void k_pg_relax_resident(PgCall a)
{
    __shared__ double s_tab[2][12 * RS_PG_RESIDENT_VIEWS];
    __shared__ uint32_t s_state[RS_PG_RESIDENT_VIEWS];
    __shared__ uint32_t s_bad[2];            // the lowest view whose net was not finite, by the parity of the round
    const uint32_t g = blockIdx.x, lane = threadIdx.x & (kPgWave - 1), w = threadIdx.x / kPgWave;
    if (a.form[g] != kPgResident) return;
    const uint32_t gs = a.graph_start[g], n = a.graph_start[g + 1] - gs;       // n <= resident_views <= RS_PG_RESIDENT_VIEWS
    for (uint32_t i = threadIdx.x; i < 12u * n; i += kPgResidentBlock) s_tab[0][i] = a.poses[(size_t)12 * gs + i];
    for (uint32_t i = threadIdx.x; i < n; i += kPgResidentBlock) s_state[i] = a.view_state[gs + i];
    if (threadIdx.x < 2) s_bad[threadIdx.x] = kPgNone;
    __syncthreads();
    uint32_t rounds = a.iterations;
    for (uint32_t round = 0; round < a.iterations; ++round) {
        const double* src = s_tab[round & 1u];
        double* dst = s_tab[(round & 1u) ^ 1u];
        for (uint32_t lv = w; lv < n; lv += RS_PG_RESIDENT_WAVES) {
            if (s_state[lv] == (uint32_t)AKZ_PG_VIEW_UPDATED) {
                if (!pg_view_round(a, src, dst, gs, gs + lv, lane) && lane == 0) {
                    s_state[lv] = AKZ_PG_VIEW_NONFINITE;
                    atomicMin(&s_bad[round & 1u], gs + lv);
                }
            } else if (lane < 12u)
                dst[12u * lv + lane] = src[12u * lv + lane];
        }
        // the one barrier of a round: dst is complete behind it; a wave that runs ahead writes the word of the other parity
        __syncthreads();
        if (s_bad[round & 1u] != kPgNone) {
            rounds = round + 1u;
            break;
        }
    }
    const double* fin = s_tab[rounds & 1u];
    for (uint32_t i = threadIdx.x; i < 12u * n; i += kPgResidentBlock) a.poses[(size_t)12 * gs + i] = fin[i];
    for (uint32_t i = threadIdx.x; i < n; i += kPgResidentBlock)
        if (s_state[i] == (uint32_t)AKZ_PG_VIEW_NONFINITE) a.view_state[gs + i] = AKZ_PG_VIEW_NONFINITE;
    if (threadIdx.x == 0) {
        const uint32_t bad = s_bad[(rounds - 1u) & 1u];          // of the last round run (iterations >= 1 here)
        a.stats[(size_t)AKZ_PG_STATS * g + AKZ_PG_S_ROUNDS] = rounds;
        a.stats[(size_t)AKZ_PG_STATS * g + AKZ_PG_S_FIRST_BAD_VIEW] = bad;
        a.graph_verdict[g] = bad != kPgNone ? AKZ_PG_NONFINITE : AKZ_PG_OK;
    }
}

// round `round` of every swept graph: reads d_poses and writes the scratch table when the round is even, the reverse when odd
__global__ __launch_bounds__(kPgBlock) void k_pg_relax_sweep(PgCall a, uint32_t round)
{
    const uint32_t lane = threadIdx.x & (kPgWave - 1), v = blockIdx.x * kPgWaves + threadIdx.x / kPgWave;
    if (v >= a.n_views) return;
    const uint32_t g = a.view_graph[v];
    if (g == kPgNone) return;
    if (a.stop[g] < round) return;                     // the graph stopped in an earlier round
    const double* src = (round & 1u) ? a.table : a.poses;
    double* dst = (round & 1u) ? a.poses : a.table;
    if (a.view_state[v] == (uint32_t)AKZ_PG_VIEW_UPDATED) {
        if (!pg_view_round(a, src, dst, 0u, v, lane) && lane == 0) {
            a.view_state[v] = AKZ_PG_VIEW_NONFINITE;
            atomicMin(&a.stats[(size_t)AKZ_PG_STATS * g + AKZ_PG_S_FIRST_BAD_VIEW], v);
            atomicMin(&a.stop[g], round);
        }
    } else if (lane < 12u)
        dst[(size_t)12 * v + lane] = src[(size_t)12 * v + lane];
}

__global__ __launch_bounds__(kPgBlock) void k_pg_finish(PgCall a)
{
    const uint32_t g = blockIdx.x;
    if (a.form[g] != kPgSweep) return;
    const uint32_t gs = a.graph_start[g], ge = a.graph_start[g + 1], stop = a.stop[g];
    const uint32_t rounds = stop == kPgNone ? a.iterations : stop + 1u;
    if (rounds & 1u)                                   // the last round landed in the scratch table
        for (size_t i = (size_t)12 * gs + threadIdx.x; i < (size_t)12 * ge; i += kPgBlock) a.poses[i] = a.table[i];
    if (threadIdx.x == 0) {
        a.stats[(size_t)AKZ_PG_STATS * g + AKZ_PG_S_ROUNDS] = rounds;
        a.graph_verdict[g] = stop == kPgNone ? AKZ_PG_OK : AKZ_PG_NONFINITE;
    }
}

}   // namespace

extern "C" int32_t rs_pose_graph_params_default(rs_pose_graph_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_pose_graph_params);
    prm->optimization_iterations = 1024;                                   // cv-sfm/src/settings.rs:461-463
    prm->graph_optimization_rate = 0.001;                                  // settings.rs:477-479
    return AKZ_OK;
}

extern "C" int32_t rs_pose_graph_debug_resident_views(rs_ctx* c, uint32_t views)
{
    if (!c || views > (uint32_t)RS_PG_RESIDENT_VIEWS) return AKZ_E_INVALID;
    rs_internal_pose_graph(c)->resident_views = views;
    return AKZ_OK;
}

extern "C" int32_t rs_pose_graph_edges_device(rs_ctx* c, const void* d_views, const void* d_constraint_poses, const void* d_constraint_verdict,
                                              uint32_t n_constraints, void* d_edges, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!c || !d_views || !d_constraint_poses || !d_constraint_verdict || !d_edges) return AKZ_E_INVALID;
        if (n_constraints == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        hipLaunchKernelGGL(k_pg_edges, dim3((n_constraints + kPgBlock - 1) / kPgBlock), dim3(kPgBlock), 0, h.stream,
                           (const double*)d_constraint_poses, (const uint32_t*)d_constraint_verdict, n_constraints, (double*)d_edges);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

// (akz_common.h) rs_pose_graph_relax_batch_device with a list of graphs to leave alone
int32_t rs_internal_pose_graph_relax(rs_ctx* c, void* d_poses, uint32_t n_views, const void* d_graph_start, uint32_t n_graphs,
                                     const void* d_row_start, const void* d_row_edges, uint32_t n_rows, const void* d_views,
                                     const void* d_constraint_verdict, const void* d_edges, uint32_t n_constraints,
                                     const rs_pose_graph_params* prm, void* d_graph_verdict, void* d_view_state, void* d_stats,
                                     const void* d_skip, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!prm || prm->struct_size != sizeof(rs_pose_graph_params)) return AKZ_E_INVALID;
        if (!AKZ_TRI_FINITE(prm->graph_optimization_rate)) return AKZ_E_INVALID;
        if (!c || !d_poses || !d_graph_start || !d_row_start || (n_rows != 0 && !d_row_edges) || !d_graph_verdict || !d_view_state || !d_stats)
            return AKZ_E_INVALID;
        if (n_constraints != 0 && (!d_views || !d_constraint_verdict || !d_edges)) return AKZ_E_INVALID;
        if (n_graphs == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        RsPoseGraphState* pg = rs_internal_pose_graph(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        // the context's scratch: the second pose table, a word per view, two per graph
        const size_t table_bytes = akz_align_up(sizeof(double) * 12 * (size_t)n_views, 256);
        const size_t view_bytes = akz_align_up(sizeof(uint32_t) * (size_t)n_views, 256);
        const size_t graph_bytes = akz_align_up(sizeof(uint32_t) * (size_t)n_graphs, 256);
        AKZ_TRY(akz_grow_scratch(h.stream, &pg->d_scratch, &pg->bytes, table_bytes + view_bytes + 2 * graph_bytes + 256));
        char* base = (char*)pg->d_scratch;
        PgCall a;
        a.poses = (double*)d_poses;
        a.table = (double*)base;
        a.view_graph = (uint32_t*)(base + table_bytes);
        a.form = (uint32_t*)(base + table_bytes + view_bytes);
        a.stop = (uint32_t*)(base + table_bytes + view_bytes + graph_bytes);
        a.graph_start = (const uint32_t*)d_graph_start;
        a.row_start = (const uint32_t*)d_row_start;
        a.row_edges = (const uint32_t*)d_row_edges;
        a.views = (const uint32_t*)d_views;
        a.cverdict = (const uint32_t*)d_constraint_verdict;
        a.edges = (const double*)d_edges;
        a.graph_verdict = (uint32_t*)d_graph_verdict;
        a.view_state = (uint32_t*)d_view_state;
        a.stats = (uint32_t*)d_stats;
        a.skip = (const uint32_t*)d_skip;
        a.n_views = n_views; a.n_graphs = n_graphs; a.n_rows = n_rows; a.n_constraints = n_constraints;
        // the bound that makes the running time finite: more iterations than RS_PG_MAX_ITERATIONS count as that
        a.iterations = prm->optimization_iterations < (uint32_t)RS_PG_MAX_ITERATIONS ? prm->optimization_iterations : (uint32_t)RS_PG_MAX_ITERATIONS;
        // A limit of at most a wave per view is a limit on the call: among more views than that the sweep's launches are
        // enqueued anyway, the resident kernel in front of them could gain nothing for its graphs and would add its time.
        a.resident_views = pg->resident_views <= (uint32_t)RS_PG_RESIDENT_WAVES && n_views > pg->resident_views ? 0u : pg->resident_views;
        a.rate = prm->graph_optimization_rate;
        if (n_views != 0) AKZ_HIP(hipMemsetAsync(a.view_graph, 0xFF, sizeof(uint32_t) * (size_t)n_views, h.stream));
        hipLaunchKernelGGL(k_pg_prepare, dim3(n_graphs), dim3(kPgBlock), 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (a.iterations == 0) return AKZ_OK;
        if (a.resident_views != 0) {
            hipLaunchKernelGGL(k_pg_relax_resident, dim3(n_graphs), dim3(kPgResidentBlock), 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        // a graph of more views than the resident form takes exists only among more views than that: the host knows no more
        // about the graphs (their sizes are device data) and asks for none
        if (n_views > a.resident_views) {
            const uint32_t grid = (n_views + kPgWaves - 1) / kPgWaves;
            for (uint32_t round = 0; round < a.iterations; ++round) {
                hipLaunchKernelGGL(k_pg_relax_sweep, dim3(grid), dim3(kPgBlock), 0, h.stream, a, round);
                AKZ_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL(k_pg_finish, dim3(n_graphs), dim3(kPgBlock), 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        return AKZ_OK;
    });
}

extern "C" int32_t rs_pose_graph_relax_batch_device(rs_ctx* c, void* d_poses, uint32_t n_views, const void* d_graph_start, uint32_t n_graphs,
                                                    const void* d_row_start, const void* d_row_edges, uint32_t n_rows, const void* d_views,
                                                    const void* d_constraint_verdict, const void* d_edges, uint32_t n_constraints,
                                                    const rs_pose_graph_params* prm, void* d_graph_verdict, void* d_view_state, void* d_stats,
                                                    void* stream_to_wait)
{
    return rs_internal_pose_graph_relax(c, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows, d_views,
                                        d_constraint_verdict, d_edges, n_constraints, prm, d_graph_verdict, d_view_state, d_stats, nullptr,
                                        stream_to_wait);
}
