// rs_export.hip — cv-sfm's export_reconstruction (cv-sfm/src/lib.rs:2285-2340, export.rs) on gfx950: the coloured point cloud
// and the cameras' frusta as the vertex arrays of the .ply file, and the file's text (rs_write_ply, host code).  An ordered
// compaction over the rows of the world table in the shape of rs_landmark_table.hip — validate, count, exclusive scan over
// tiles of RS_LT_TILE rows, scatter — and one reduction per view, the one of k_nr_normalize; every decision and all the
// arithmetic is include/akz_export_math.h, the text the CPU checker (tests/cpp/export_host.c) compiles too — parity: host
// build == HIP, byte for byte.
//
// rs_export_reconstruction_device, in stream order:
//   k_ex_check      one lane per start: do the starts begin at 0 and ascend inside [0, n_obs].
//   k_ex_tile_sums  first level of the scan: one lane per row says what the row is (akz_ex_row), one workgroup per tile counts
//                   its tile's points; the rows that are skipped are counted by their kind.
//   k_ex_scan_sums  second level: ONE workgroup walks the tile sums kTblBlock at a time behind a running carry; the counts and
//                   the verdict.
//   k_ex_points     third pass: a workgroup scans its tile again; the lane of a point below the room does the three divisions,
//                   gathers the colour of the first observation and writes the key.
//   k_ex_cameras    one workgroup of 256 per view: the mean distance in include/akz_sum_order.h's order, the camera row and its
//                   five vertices.
// Nothing here waits on a value another workgroup has yet to write: the levels are separate launches; every loop is bounded by
// an argument.  The call shares the scratch rs_landmark_table.hip keeps in the context: the calls run on one stream.
#include <stdio.h>

#include "rs_table.h"
#include "../../include/akz_export_math.h"

namespace {

static_assert(kTblBlock == AKZ_SUM_THREADS, "the workgroup akz_sum_order.h's T = 256 stands for");

static_assert(RS_EX_OK == AKZ_EX_OK && RS_EX_OVERFLOW == AKZ_EX_OVERFLOW && RS_EX_BAD_TABLE == AKZ_EX_BAD_TABLE, "verdicts");
static_assert(RS_EX_C_POINTS == AKZ_EX_C_POINTS && RS_EX_C_NO_POINT == AKZ_EX_C_NO_POINT && RS_EX_C_INFINITE == AKZ_EX_C_INFINITE &&
              RS_EX_C_BAD_ROWS == AKZ_EX_C_BAD_ROWS && RS_EX_COUNTS == AKZ_EX_COUNTS, "count words");
static_assert(RS_EX_CAMERA_WORDS == AKZ_EX_CAMERA_WORDS && RS_EX_CAMERA_VERTICES == AKZ_EX_CAMERA_VERTICES, "camera shapes");
static_assert(AKZ_EX_ROW_POINT == AKZ_EX_C_POINTS && AKZ_EX_ROW_NO_POINT == AKZ_EX_C_NO_POINT && AKZ_EX_ROW_INFINITE == AKZ_EX_C_INFINITE &&
              AKZ_EX_ROW_BAD == AKZ_EX_C_BAD_ROWS, "a row's kind is the word of its count");

// words of ExCall::info: [0, AKZ_EX_COUNTS) the rows of each kind, then
enum { kExBadTable = AKZ_EX_COUNTS, kExInfoWords = 8 };

// everything the kernels of one call share, by value
struct ExCall {
    const double* world;          // [n_world][4]
    const uint32_t* start;        // [n_landmarks + 1]
    const uint32_t* obs;          // [n_obs][2]
    const uint8_t* colors;        // [n_blocks][cap][3]
    const uint32_t* counts;       // [n_blocks]
    const uint32_t* landmarks;    // [n_blocks][cap]
    const double* poses;          // [n_blocks][12]
    double* xyz;                  // [5 * n_views + room][3]
    uint8_t* rgb;                 // [5 * n_views + room][3]
    uint32_t* key;                // [room]
    double* cameras;              // [n_views][AKZ_EX_CAMERA_WORDS]
    uint32_t* counts_out;         // [AKZ_EX_COUNTS]
    uint32_t* verdict;            // [1]
    // scratch
    uint32_t* info;               // [kExInfoWords]
    uint32_t* tile_points;        // [n_tiles] a tile's points, then the points in front of it
    uint32_t* views;              // [n_views] view_blocks
    uint32_t n_world, n_landmarks, n_obs, cap, n_blocks, n_views, room, n_tiles;
};

// info is zero in front of it
__global__ __launch_bounds__(kTblBlock) void k_ex_check(ExCall a)
{
    const uint32_t l = blockIdx.x * kTblBlock + threadIdx.x;
    const int bad = l <= a.n_landmarks && akz_ex_start_bad(a.start, l, a.n_landmarks, a.n_obs);
    tbl_flag(&a.info[kExBadTable], bad);
}

// what row r is to the call; a refused table has no row
__device__ __forceinline__ uint32_t ex_row(const ExCall& a, bool ok, uint32_t r, uint32_t* block, uint32_t* feature)
{
    if (!ok || r >= a.n_world) return AKZ_EX_COUNTS;
    return akz_ex_row(a.world, a.start, a.obs, r, a.n_landmarks, a.n_obs, a.n_blocks, a.cap, block, feature);
}

__global__ __launch_bounds__(kTblBlock) void k_ex_tile_sums(ExCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    const bool ok = a.info[kExBadTable] == 0u;
    uint32_t n[AKZ_EX_COUNTS] = {0u, 0u, 0u, 0u}, tick = 0u;
#pragma unroll
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;       // n_world + kTblTile < 2^32: the entry point
        uint32_t blk, feat;
        const uint32_t what = ex_row(a, ok, r, &blk, &feat);
#pragma unroll
        for (int k = 0; k < AKZ_EX_COUNTS; ++k) n[k] += what == (uint32_t)k ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < AKZ_EX_COUNTS; ++k) n[k] = akz_block_sum<kTblWaves>(s_cnt, tick, n[k]);
    if (threadIdx.x == 0) {
        a.tile_points[blockIdx.x] = n[AKZ_EX_C_POINTS];
#pragma unroll
        for (int k = 0; k < AKZ_EX_COUNTS; ++k)
            if (n[k]) atomicAdd(&a.info[k], n[k]);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_ex_scan_sums(ExCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t carry = tbl_scan_in_place(a.tile_points, a.n_tiles, s_wave);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < AKZ_EX_COUNTS; ++k) a.counts_out[k] = a.info[k];                   // carry == info[AKZ_EX_C_POINTS]
        *a.verdict = akz_ex_verdict(a.info[kExBadTable] != 0u, carry, a.room);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_ex_points(ExCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const bool ok = a.info[kExBadTable] == 0u;
    const size_t first = (size_t)AKZ_EX_CAMERA_VERTICES * a.n_views;
    uint32_t run = a.tile_points[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;
        uint32_t blk = 0u, feat = 0u;
        const bool point = ex_row(a, ok, r, &blk, &feat) == (uint32_t)AKZ_EX_ROW_POINT;
        const uint32_t k = tbl_scan_step(run, point ? 1u : 0u, s_wave);
        if (point && k < a.room) {                           // blk < n_blocks and feat < cap: akz_ex_row
            const size_t at = first + k;
            double p[3];
            akz_ex_point(a.world + 4 * (size_t)r, p);
            const uint8_t* c = a.colors + 3 * ((size_t)blk * a.cap + feat);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a.xyz[3 * at + i] = p[i];
                a.rgb[3 * at + i] = c[i];
            }
            a.key[k] = r;
        }
    }
}

// one workgroup of AKZ_SUM_THREADS per view
__global__ __launch_bounds__(kTblBlock) void k_ex_cameras(ExCall a)
{
    __shared__ double s_red[2][kTblWaves][1];
    __shared__ uint32_t s_cnt[2][kTblWaves];
    const uint32_t v = blockIdx.x, block = a.views[v];       // block < n_blocks: the entry point
    const uint32_t count = akz_ex_count(a.counts[block], a.cap);
    double pose[12];
    for (int k = 0; k < 12; ++k) pose[k] = a.poses[(size_t)12 * block + k];
    double part[1] = {0.0}, net[1];
    uint32_t n = 0u, tick = 0u;
    for (uint32_t j = threadIdx.x; j < count; j += kTblBlock) {
        double d;
        if (!akz_ex_feature_distance(pose, a.landmarks + (size_t)block * a.cap, j, a.world, a.n_world, &d)) continue;
        part[0] = part[0] + d;
        ++n;
    }
    akz_block_sum<kTblWaves, 1>(s_red, 0u, part, net);
    n = akz_block_sum<kTblWaves>(s_cnt, tick, n);
    // every thread holds the same bits: the lanes that hold a word write it
    const uint32_t t = threadIdx.x;
    if (t >= 3u * AKZ_EX_CAMERA_VERTICES) return;
    double cam[AKZ_EX_CAMERA_WORDS], vert[3];
    akz_ex_camera(pose, akz_nr_mean(net[0], n), cam);
    if (t < (uint32_t)AKZ_EX_CAMERA_WORDS) a.cameras[(size_t)AKZ_EX_CAMERA_WORDS * v + t] = cam[t];
    const uint32_t k = t / 3u, i = t - 3u * k;
    akz_ex_camera_vertex(cam, (int)k, vert);
    const size_t at = 3 * ((size_t)AKZ_EX_CAMERA_VERTICES * v + k) + i;
    a.xyz[at] = vert[i];
    a.rgb[at] = akz_ex_camera_color((int)i);
}

}   // namespace

extern "C" int32_t rs_export_reconstruction_device(rs_ctx* c, const void* d_world, uint32_t n_world, const void* d_obs_start, const void* d_obs,
                                                   uint32_t n_obs, uint32_t n_landmarks, const void* d_colors, const uint32_t* view_blocks,
                                                   uint32_t n_views, const void* d_counts, const void* d_landmarks, uint32_t cap_per_img,
                                                   uint32_t n_blocks, const void* d_poses, uint32_t room, void* d_xyz, void* d_rgb, void* d_key,
                                                   void* d_cameras, void* d_counts_out, void* d_verdict, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if ((n_world != 0 && !d_world) || !d_obs_start || (n_obs != 0 && !d_obs) || !d_colors || !view_blocks || !d_counts || !d_landmarks ||
            !d_poses || !d_xyz || !d_rgb || (room != 0 && !d_key) || !d_cameras || !d_counts_out || !d_verdict)
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || n_views == 0) return AKZ_E_INVALID;
        // row numbers of the last tile, start numbers of the last workgroup and vertex numbers stay 32-bit
        if (n_world > 0xFFFFFFFFu - 2u * kTblTile || n_landmarks > 0xFFFFFFFFu - 2u * kTblBlock ||
            (uint64_t)AKZ_EX_CAMERA_VERTICES * n_views + room > 0xFFFFFFFFull)
            return AKZ_E_TOO_LARGE;
        // two workgroups never write one camera: the blocks are distinct and inside the table
        std::vector<unsigned char> seen;
        if (!akz_distinct_blocks(view_blocks, n_views, n_blocks, &seen)) return AKZ_E_INVALID;
        // the inputs are const: no output may lie over them
        const size_t n_vertices = (size_t)AKZ_EX_CAMERA_VERTICES * n_views + room, features = (size_t)n_blocks * cap_per_img;
        const void* in[7] = {d_world, d_obs_start, d_obs, d_colors, d_counts, d_landmarks, d_poses};
        const size_t in_bytes[7] = {sizeof(double) * 4 * (size_t)n_world, sizeof(uint32_t) * ((size_t)n_landmarks + 1), sizeof(uint32_t) * 2 * (size_t)n_obs,
                                    3 * features, sizeof(uint32_t) * (size_t)n_blocks, sizeof(uint32_t) * features, sizeof(double) * 12 * (size_t)n_blocks};
        const void* out[6] = {d_xyz, d_rgb, d_key, d_cameras, d_counts_out, d_verdict};
        const size_t out_bytes[6] = {sizeof(double) * 3 * n_vertices, 3 * n_vertices, sizeof(uint32_t) * (size_t)room,
                                     sizeof(double) * AKZ_EX_CAMERA_WORDS * (size_t)n_views, sizeof(uint32_t) * AKZ_EX_COUNTS, sizeof(uint32_t)};
        if (!akz_outputs_clear_of_inputs(in, in_bytes, 7, out, out_bytes, 6)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        const uint32_t n_tiles = (uint32_t)(((size_t)n_world + kTblTile - 1) / kTblTile);
        const size_t w = sizeof(uint32_t);
        AkzScratchPlan plan;
        const size_t at_info = plan.take(w * kExInfoWords), at_tiles = plan.take(w * ((size_t)n_tiles + 1)), at_views = plan.take(w * (size_t)n_views);
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, plan.size()));
        char* base = (char*)ls->d_scratch;
        ExCall a;
        a.world = (const double*)d_world; a.start = (const uint32_t*)d_obs_start; a.obs = (const uint32_t*)d_obs; a.colors = (const uint8_t*)d_colors;
        a.counts = (const uint32_t*)d_counts; a.landmarks = (const uint32_t*)d_landmarks; a.poses = (const double*)d_poses;
        a.xyz = (double*)d_xyz; a.rgb = (uint8_t*)d_rgb; a.key = (uint32_t*)d_key; a.cameras = (double*)d_cameras;
        a.counts_out = (uint32_t*)d_counts_out; a.verdict = (uint32_t*)d_verdict;
        a.info = (uint32_t*)(base + at_info); a.tile_points = (uint32_t*)(base + at_tiles); a.views = (uint32_t*)(base + at_views);
        a.n_world = n_world; a.n_landmarks = n_landmarks; a.n_obs = n_obs; a.cap = cap_per_img; a.n_blocks = n_blocks; a.n_views = n_views;
        a.room = room; a.n_tiles = n_tiles;
        AKZ_HIP(hipMemsetAsync(base + at_info, 0, at_tiles - at_info, h.stream));
        AKZ_HIP(hipMemcpyAsync(a.views, view_blocks, w * n_views, hipMemcpyHostToDevice, h.stream));
        const dim3 block(kTblBlock);
        hipLaunchKernelGGL(k_ex_check, dim3(n_landmarks / kTblBlock + 1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_tiles) {
            hipLaunchKernelGGL(k_ex_tile_sums, dim3(n_tiles), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_ex_scan_sums, dim3(1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_tiles) {
            hipLaunchKernelGGL(k_ex_points, dim3(n_tiles), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_ex_cameras, dim3(n_views), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

// export.rs:22-137 with ply-rs' ASCII writer (not in the tree: its number text and line ends are unpinned): numbers
// as %.17g, which a reader turns back into the same f64 bits, lines ended by \n.
extern "C" int32_t rs_write_ply(const char* path, const double* xyz, const uint8_t* rgb, uint32_t n_vertices, uint32_t n_cameras,
                                int32_t camera_faces)
{
    return akz_guard([&]() -> int32_t {
        if (!path || (n_vertices != 0 && (!xyz || !rgb)) || (uint64_t)AKZ_EX_CAMERA_VERTICES * n_cameras > n_vertices) return AKZ_E_INVALID;
        FILE* fp = fopen(path, "w");
        if (!fp) return AKZ_E_INVALID;
        fprintf(fp, "ply\nformat ascii 1.0\ncomment Exported from rust-cv/vslam-sandbox\nelement vertex %u\n", (unsigned)n_vertices);
        fprintf(fp, "property double x\nproperty double y\nproperty double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n");
        if (camera_faces) fprintf(fp, "element face %llu\nproperty list uchar int vertex_index\n", 4ull * n_cameras);
        fprintf(fp, "end_header\n");
        for (size_t i = 0; i < n_vertices; ++i)
            fprintf(fp, "%.17g %.17g %.17g %u %u %u\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (unsigned)rgb[3 * i], (unsigned)rgb[3 * i + 1],
                    (unsigned)rgb[3 * i + 2]);
        if (camera_faces)
            for (uint32_t v = 0; v < n_cameras; ++v) {
                // centre b, up-right b + 1, up-left b + 2, down-left b + 3, down-right b + 4 (export.rs:108-113)
                const unsigned long long b = (unsigned long long)AKZ_EX_CAMERA_VERTICES * v;
                fprintf(fp, "3 %llu %llu %llu\n3 %llu %llu %llu\n3 %llu %llu %llu\n3 %llu %llu %llu\n", b, b + 4, b + 1, b, b + 1, b + 2, b, b + 2,
                        b + 3, b, b + 3, b + 4);
            }
        const bool failed = ferror(fp) != 0;
        return (fclose(fp) != 0 || failed) ? AKZ_E_INVALID : AKZ_OK;
    });
}
