// vmap_search.hip -- the exhaustive lattice pose search over the voxel map (slam_vmap_search*, docs/VOXEL_MAP.md section 13):
// "here is a scan, here is the map, where am I?" without a prior.  For one rotation the scan's cells are computed once; a
// translation by whole cells moves every point's cell by the same integers, so a pose's score is a count of set bits in a
// dense occupancy brick at integer offsets.  Behind the cells there is no floating point, and an integer sum is the same
// bits in any order.  The restatement is tests/vmap_search_cases.py.
//   vmap_search_cells_kernel   one lane per (point, rotation): the point moved by moved_point, its cell by vmap_point_cell --
//                              the functions integrate uses, and the only floating point here -- or the "no cell" mark; the
//                              integer box of the cells by atomicMin / atomicMax and a count of the points with a cell a
//                              rotation, both reduced over the wavefront first.
//   vmap_search_brick_kernel   one lane per table slot: a qualifying voxel inside the box widened by the window sets its bit
//                              with an integer atomicOr.  The brick carries the window as a margin on every side, so c + d
//                              never leaves it; behind it lies as much again of zeros, where the points without a cell point,
//                              so the scoring loop has neither a bounds test nor a branch.
//   vmap_search_score_kernel   the hot path.  A workgroup takes one rotation, 64 consecutive dx and four (dz, dy) rows, one a
//                              wavefront: the lanes of a wavefront are the dx, so its loads for one point fall in two or three
//                              adjacent words.  The rotation's cells become linear bit indices as they are staged in LDS,
//                              8 192 at a time (32 KB); the loop reads one per point and does one load, a shift, an and, an
//                              add, eight points in flight.  One plain store per pose; no atomics; no lane waits on another.
//                              (Four rows a lane instead of one measured half as fast at the default shape: a quarter of the
//                              wavefronts.)
//                              The brick is read through the cache hierarchy: held in LDS where it fits, the kernel measured
//                              9 % slower at the default shape (docs/VOXEL_MAP.md section 13.3), so that form is not kept.
//   vmap_search_best_kernel /  top_m rounds of a two-stage arg-max over the volume with the key score << 32 | ~flat (the lowest
//   vmap_search_pick_kernel    flat index wins a tie); a pose inside the box of an earlier hit, read from the device's own
//                              hit list, is passed over.
// The host waits twice: for the box, which sizes the brick, and for the hits.
#include <climits>
#include <cmath>
#include <cstring>

#include "kf_common.hpp"
#include "vmap_dist.hpp"

namespace {

constexpr int      kNoCell = INT_MIN;       // in the x plane of the cells: the point has no cell under this rotation
constexpr int      kStage = 8192;           // bit indices staged in LDS at a time
constexpr int      kUnroll = 8;             // points in flight: eight loads a lane
constexpr int      kScoreThreads = 256;     // four wavefronts: four rows a workgroup
constexpr int      kTileRows = kScoreThreads / 64;
constexpr int      kBestBlocks = 1024;      // partial maxima of the first arg-max stage, at most
constexpr int      kMaxHits = 4096;
constexpr int64_t  kMaxPoses = 1ll << 26;
constexpr int64_t  kMaxBrickBits = 1ll << 31;
constexpr int      kHitWords = 8;           // a hit on the device: score, k, dx, dy, dz, n_with_cell, two spare

// the block `small`, in 32-bit words: the box (min x y z, max x y z), the hit count, a spare; then the hits, the partial
// maxima (u64 each) and the points with a cell per rotation
enum { kBoxMin = 0, kBoxMax = 3, kHitCount = 6, kHeadWords = 8 };

struct Window {
    int wx, wy, wz, n_yaw;
    int dx, dy, dz; // 2 w + 1
};

// the brick: bit ((z - o.z) Y + (y - o.y)) X + (x - o.x) for a cell inside [o, o + (X, Y, Z))
struct Brick {
    int      o[3];
    uint32_t X, Y, Z;
    uint32_t null_bit; // where a point without a cell points: every offset from it lands in the zeros behind the brick
};

struct Nms {
    int yaw, cells;
};

__global__ __launch_bounds__(256) void vmap_search_cells_kernel(const float *xyz, int n, int stride, const VmapTransform *rot, int n_yaw, double leaf,
                                                                int32_t *cells, int32_t *box, uint32_t *with_cell)
{
    __shared__ int sBox[6];
    const int tid = threadIdx.x;
    if (tid < 3) sBox[tid] = INT_MAX, sBox[3 + tid] = INT_MIN;
    __syncthreads();
    const size_t total = (size_t)n * n_yaw, at = (size_t)blockIdx.x * 256 + tid;
    bool         has = false;
    int          c[3] = {0, 0, 0}, k = 0;
    if (at < total) {
        k = (int)(at / n);
        float q[3];
        moved_point(xyz + (at - (size_t)k * n) * stride, rot[k], q);
        has = vmap_point_cell(q, leaf, c);
        cells[at] = has ? c[0] : kNoCell, cells[total + at] = c[1], cells[2 * total + at] = c[2];
    }
    // The wavefront's box and count first, then one atomic a wavefront: a lane's own atomicAdd on its rotation's word had
    // every point of a rotation queue at one address (1.6 ms of a 2.1 ms search at the default shape).
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = has ? c[a] : INT_MAX, hi[a] = has ? c[a] : INT_MIN;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int l = __shfl_xor(lo[a], s), h = __shfl_xor(hi[a], s);
            lo[a] = l < lo[a] ? l : lo[a], hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    // the lanes of the wavefront's first rotation are counted by one ballot; a wavefront that straddles rotations has a few more
    const int                k0 = __builtin_amdgcn_readfirstlane(k); // a lane past the end has k = 0 and no cell
    const unsigned long long same = __ballot(has && k == k0);
    if ((tid & 63) == 0) {
        if (same) atomicAdd(&with_cell[k0], (uint32_t)__popcll(same));
        if (lo[0] <= hi[0]) {
#pragma unroll
            for (int a = 0; a < 3; ++a) atomicMin(&sBox[a], lo[a]), atomicMax(&sBox[3 + a], hi[a]);
        }
    }
    if (has && k != k0) atomicAdd(&with_cell[k], 1u);
    __syncthreads();
    if (tid < 3 && sBox[tid] <= sBox[3 + tid]) atomicMin(&box[kBoxMin + tid], sBox[tid]), atomicMax(&box[kBoxMax + tid], sBox[3 + tid]);
}

__global__ __launch_bounds__(256) void vmap_search_brick_kernel(VmapSearchView V, Brick B, uint32_t min_count, uint32_t *brick)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > V.mask) return;
    int c[3];
    if (!vmap_key_cell(V.key[i], c)) return; // an empty slot
    const bool is = V.cen ? V.cen[i].w == 1.0f : V.count[i] >= min_count;
    if (!is) return;
    const uint32_t x = (uint32_t)(c[0] - B.o[0]), y = (uint32_t)(c[1] - B.o[1]), z = (uint32_t)(c[2] - B.o[2]); // a cell below o wraps far above
    if (x >= B.X || y >= B.Y || z >= B.Z) return;
    const uint32_t bit = (z * B.Y + y) * B.X + x;
    atomicOr(&brick[bit >> 5], 1u << (bit & 31u));
}

__global__ __launch_bounds__(kScoreThreads) void vmap_search_score_kernel(const int32_t *cells, int n, Window W, Brick B, const uint32_t *brick,
                                                                          int32_t *volume)
{
    __shared__ uint32_t sBit[kStage];
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int      rows = W.dz * W.dy;
    const uint32_t x_tiles = (uint32_t)(W.dx + 63) / 64, row_tiles = (uint32_t)(rows + kTileRows - 1) / kTileRows;
    const uint32_t xt = blockIdx.x % x_tiles, rt = blockIdx.x / x_tiles % row_tiles, k = blockIdx.x / x_tiles / row_tiles;
    // a lane past the window's edge, or a wavefront past the last row, works on the edge's pose and stores nothing: its
    // offsets stay inside the margin and it meets every barrier
    const int      xi = (int)xt * 64 + lane, xc = xi < W.dx ? xi : W.dx - 1;
    const int      row = (int)rt * kTileRows + wave, r = row < rows ? row : rows - 1;
    const int      dz = r / W.dy - W.wz, dy = r % W.dy - W.wy;
    const uint32_t off = (uint32_t)((dz * (int)B.Y + dy) * (int)B.X + (xc - W.wx));
    int            acc = 0;
    const size_t   total = (size_t)n * W.n_yaw;
    const int32_t *cx = cells + (size_t)k * n, *cy = cx + total, *cz = cy + total;
    for (int first = 0; first < n; first += kStage) {
        const int m = n - first < kStage ? n - first : kStage;
        __syncthreads();
        for (int i = tid; i < m; i += kScoreThreads) {
            const int x = cx[first + i];
            sBit[i] = x == kNoCell ? B.null_bit
                                   : ((uint32_t)(cz[first + i] - B.o[2]) * B.Y + (uint32_t)(cy[first + i] - B.o[1])) * B.X + (uint32_t)(x - B.o[0]);
        }
        __syncthreads();
#pragma unroll kUnroll
        for (int i = 0; i < m; ++i) { // the points are independent of each other: kUnroll loads in flight a lane
            const uint32_t bit = sBit[i] + off;
            acc += (int)((brick[bit >> 5] >> (bit & 31u)) & 1u);
        }
    }
    if (xi < W.dx && row < rows) volume[((size_t)k * rows + row) * W.dx + xi] = acc;
}

// is the pose `flat` inside the box of one of the first `n_hits` hits
__device__ __forceinline__ bool suppressed(uint32_t flat, const Window &W, const Nms &N, const int32_t *hit, int n_hits)
{
    const int x = (int)(flat % W.dx) - W.wx, y = (int)(flat / W.dx % W.dy) - W.wy, z = (int)(flat / W.dx / W.dy % W.dz) - W.wz;
    const int k = (int)(flat / W.dx / W.dy / W.dz);
    for (int h = 0; h < n_hits; ++h) {
        const int32_t *H = hit + kHitWords * h;
        int            dk = abs(k - H[1]);
        dk = dk < W.n_yaw - dk ? dk : W.n_yaw - dk; // cyclic
        if (dk <= N.yaw && abs(x - H[2]) <= N.cells && abs(y - H[3]) <= N.cells && abs(z - H[4]) <= N.cells) return true;
    }
    return false;
}

__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// stage one of a round: every workgroup's best key among the poses of score > 0 that no earlier hit suppresses (0: none)
__global__ __launch_bounds__(256) void vmap_search_best_kernel(const int32_t *volume, uint32_t poses, Window W, Nms N, const int32_t *head, int max_hits,
                                                               unsigned long long *partial)
{
    __shared__ unsigned long long red[256];
    __shared__ int32_t            sHit[kHitWords * 64]; // the earlier hits, 64 at a time
    const int          n_hits = head[kHitCount] < max_hits ? head[kHitCount] : max_hits;
    const int32_t     *hit = head + kHeadWords;
    unsigned long long best = 0;
    // the hits in LDS while they fit; beyond 64 they are read where they lie
    const int in_lds = n_hits < 64 ? n_hits : 64;
    for (int i = threadIdx.x; i < kHitWords * in_lds; i += 256) sHit[i] = hit[i];
    __syncthreads();
    for (uint32_t flat = blockIdx.x * 256u + threadIdx.x; flat < poses; flat += gridDim.x * 256u) {
        const int s = volume[flat];
        if (s <= 0) continue;
        const unsigned long long key = (unsigned long long)(uint32_t)s << 32 | (uint32_t)~flat;
        if (key <= best) continue;
        if (suppressed(flat, W, N, sHit, in_lds) || suppressed(flat, W, N, hit + kHitWords * in_lds, n_hits - in_lds)) continue;
        best = key;
    }
    best = block_max(best, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// stage two: the best of the partial maxima becomes the next hit, or nothing when no pose is left
__global__ __launch_bounds__(256) void vmap_search_pick_kernel(const unsigned long long *partial, int n_partial, Window W, const uint32_t *with_cell,
                                                               int32_t *head, int max_hits)
{
    __shared__ unsigned long long red[256];
    unsigned long long best = 0;
    for (int i = threadIdx.x; i < n_partial; i += 256) best = partial[i] > best ? partial[i] : best;
    best = block_max(best, red);
    if (threadIdx.x != 0 || best == 0 || head[kHitCount] >= max_hits) return;
    const uint32_t flat = ~(uint32_t)best;
    int32_t       *H = head + kHeadWords + kHitWords * head[kHitCount];
    H[0] = (int32_t)(best >> 32);
    H[1] = (int32_t)(flat / W.dx / W.dy / W.dz);
    H[2] = (int32_t)(flat % W.dx) - W.wx, H[3] = (int32_t)(flat / W.dx % W.dy) - W.wy, H[4] = (int32_t)(flat / W.dx / W.dy % W.dz) - W.wz;
    H[5] = (int32_t)with_cell[H[1]], H[6] = H[7] = 0;
    head[kHitCount] += 1;
}

// yaw_k and the f32 matrix planar(x, y, yaw_k) with z as its z translation, as MapLocalizer::yawFan and GlobalMatcher::planar
// build theirs: cos and sin in double of the float angle, rounded to float
void planar_k(const slam_vmap_search_params &p, int k, float x, float y, float z, float M[16])
{
    const float yaw = (float)((double)p.yaw0 + 2.0 * M_PI * (double)k / (double)p.n_yaw);
    const float c = (float)std::cos((double)yaw), s = (float)std::sin((double)yaw);
    const float m[16] = {c, -s, 0, x, s, c, 0, y, 0, 0, 1, z, 0, 0, 0, 1};
    for (int e = 0; e < 16; ++e) M[e] = m[e];
}

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int check_search(const char *who, slam_vmap_t *m, const void *xyz, int n, int stride, const slam_vmap_search_params &p, const void *hits,
                 const int *n_hits)
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "%s: map is NULL", who);
    SLAM_REQUIRE(n >= 0 && stride >= 3 && (xyz || n == 0), SLAM_E_INVALID, "%s: n >= 0, stride >= 3 and points", who);
    SLAM_REQUIRE(p.n_yaw >= 1 && p.wx >= 0 && p.wy >= 0 && p.wz >= 0, SLAM_E_INVALID, "%s: n_yaw >= 1 and half-widths >= 0", who);
    SLAM_REQUIRE(p.top_m >= 0 && p.top_m <= kMaxHits && p.nms_yaw >= 0 && p.nms_cells >= 0, SLAM_E_INVALID,
                 "%s: top_m in 0 .. %d, nms_yaw and nms_cells >= 0", who, kMaxHits);
    SLAM_REQUIRE(n_hits && (hits || p.top_m == 0), SLAM_E_INVALID, "%s: n_hits, and hits with top_m > 0", who);
    int64_t poses = p.n_yaw; // each factor is below 2^32 and the product is tested after each: no overflow
    for (const int w : {p.wx, p.wy, p.wz}) {
        if (poses <= kMaxPoses) poses *= 2 * (int64_t)w + 1;
    }
    SLAM_REQUIRE(poses <= kMaxPoses, SLAM_E_INVALID, "%s: n_yaw (2 wx + 1)(2 wy + 1)(2 wz + 1) is more than the 2^26 poses a call may score", who);
    return SLAM_OK;
}

// The one launch path: `d_xyz` are n device points `stride` floats apart, the arguments have passed check_search.
int search_launch(const char *who, slam_vmap_t *m, const float *d_xyz, int n, int stride, const slam_vmap_search_params &p,
                  slam_vmap_search_hit *hits, int *n_hits, int32_t *volume, hipStream_t st)
{
    Window W;
    W.wx = p.wx, W.wy = p.wy, W.wz = p.wz, W.n_yaw = p.n_yaw;
    W.dx = 2 * p.wx + 1, W.dy = 2 * p.wy + 1, W.dz = 2 * p.wz + 1;
    const size_t poses = (size_t)W.n_yaw * W.dz * W.dy * W.dx;
    *n_hits = 0;
    VmapSearchView V;
    SLAM_TRY(vmap_search_view(m, p.planes_only != 0, st, &V)); // refuses planes_only without distributions
    if (V.n_voxels == 0 || n == 0) { // nothing to count: a zero volume, no hits
        if (volume) std::memset(volume, 0, poses * sizeof(int32_t));
        return SLAM_OK;
    }
    VmapSearchWork &K = vmap_search_work(m);
    const size_t    total = (size_t)n * W.n_yaw;
    const int       n_partial = (int)std::min<size_t>((poses + 255) / 256, kBestBlocks);
    // small: head | hits | partials | with_cell; pinned: the rotations | head and hits
    const size_t hit_off = kHeadWords * 4, part_off = up256(hit_off + (size_t)kHitWords * 4 * p.top_m), cell_off = part_off + up256(8 * (size_t)n_partial);
    const size_t small_b = cell_off + 4 * (size_t)W.n_yaw, rot_b = sizeof(VmapTransform) * (size_t)W.n_yaw, back_b = part_off;
    SLAM_TRY(reserve_quarter(K.small, small_b));
    SLAM_TRY(reserve_quarter(K.rot, rot_b));
    SLAM_TRY(reserve_quarter(K.cells, 3 * total * sizeof(int32_t)));
    char *host = static_cast<char *>(pinned_scratch(up256(rot_b) + back_b));
    SLAM_REQUIRE(host, SLAM_E_NOMEM, "%s: no pinned staging memory", who);
    VmapTransform *rot = reinterpret_cast<VmapTransform *>(host);
    int32_t       *back = reinterpret_cast<int32_t *>(host + up256(rot_b));
    for (int k = 0; k < W.n_yaw; ++k) {
        float M[16];
        planar_k(p, k, p.cx, p.cy, p.cz, M);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) rot[k].r[3 * r + c] = (double)M[4 * r + c];
            rot[k].t[r] = (double)M[4 * r + 3];
        }
        rot[k].on = 1;
    }
    for (int a = 0; a < 3; ++a) back[kBoxMin + a] = INT_MAX, back[kBoxMax + a] = INT_MIN;
    back[kHitCount] = back[kHitCount + 1] = 0;
    char *small = K.small.as<char>();
    SLAM_HIP(hipMemcpyAsync(K.rot.p, rot, rot_b, hipMemcpyHostToDevice, st));
    SLAM_HIP(hipMemcpyAsync(small, back, hit_off, hipMemcpyHostToDevice, st));
    SLAM_HIP(hipMemsetAsync(small + cell_off, 0, 4 * (size_t)W.n_yaw, st));
    int32_t  *head = reinterpret_cast<int32_t *>(small);
    uint32_t *with_cell = reinterpret_cast<uint32_t *>(small + cell_off);
    hipLaunchKernelGGL(vmap_search_cells_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_xyz, n, stride, K.rot.as<VmapTransform>(),
                       W.n_yaw, V.leaf, K.cells.as<int32_t>(), head, with_cell);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(back, small, hit_off, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st)); // the first wait: the box of the moved cells
    if (back[kBoxMin] > back[kBoxMax]) { // no point has a cell under any rotation
        if (volume) std::memset(volume, 0, poses * sizeof(int32_t));
        return SLAM_OK;
    }
    Brick   B;
    int64_t dim[3];
    const int w[3] = {p.wx, p.wy, p.wz};
    for (int a = 0; a < 3; ++a) {
        B.o[a] = back[kBoxMin + a] - w[a]; // |cell| < 2^20 and w < 2^25: no overflow
        dim[a] = (int64_t)back[kBoxMax + a] - back[kBoxMin + a] + 1 + 2 * (int64_t)w[a];
    }
    // Every dim is below 2^27, so a plane is below 2^54; it is tested before it is multiplied again.  `reach` is the far
    // corner's offset: a point without a cell points that far behind the brick, and as far again is zeros.
    const int64_t plane = dim[0] * dim[1], fits = plane <= kMaxBrickBits;
    const int64_t bits = fits ? plane * dim[2] : 0, reach = fits ? (int64_t)p.wz * plane + (int64_t)p.wy * dim[0] + p.wx : 0;
    SLAM_REQUIRE(fits && bits + 2 * reach + 64 <= kMaxBrickBits, SLAM_E_NOMEM,
                 "%s: the box of the moved cells plus the window is %lld x %lld x %lld cells: more than the 2^31 bits a brick may have", who,
                 (long long)dim[0], (long long)dim[1], (long long)dim[2]);
    B.X = (uint32_t)dim[0], B.Y = (uint32_t)dim[1], B.Z = (uint32_t)dim[2];
    B.null_bit = (uint32_t)(bits + reach);
    const size_t brick_b = (size_t)((bits + 2 * reach + 64) / 32) * 4;
    SLAM_TRY(reserve_quarter(K.brick, brick_b));
    SLAM_TRY(reserve_quarter(K.volume, poses * sizeof(int32_t)));
    SLAM_HIP(hipMemsetAsync(K.brick.p, 0, brick_b, st));
    hipLaunchKernelGGL(vmap_search_brick_kernel, dim3((unsigned)((V.mask + 256) / 256)), dim3(256), 0, st, V, B, (uint32_t)std::max(p.min_count, 0),
                       K.brick.as<uint32_t>());
    SLAM_HIP(hipGetLastError());
    const unsigned x_tiles = (unsigned)(W.dx + 63) / 64, row_tiles = (unsigned)(W.dz * W.dy + kTileRows - 1) / kTileRows;
    hipLaunchKernelGGL(vmap_search_score_kernel, dim3(x_tiles * row_tiles * (unsigned)W.n_yaw), dim3(kScoreThreads), 0, st, K.cells.as<int32_t>(), n, W, B,
                       K.brick.as<uint32_t>(), K.volume.as<int32_t>());
    SLAM_HIP(hipGetLastError());
    Nms                 N{p.nms_yaw, p.nms_cells};
    unsigned long long *partial = reinterpret_cast<unsigned long long *>(small + part_off);
    for (int round = 0; round < p.top_m; ++round) {
        hipLaunchKernelGGL(vmap_search_best_kernel, dim3(n_partial), dim3(256), 0, st, K.volume.as<int32_t>(), (uint32_t)poses, W, N, head, p.top_m, partial);
        hipLaunchKernelGGL(vmap_search_pick_kernel, dim3(1), dim3(256), 0, st, partial, n_partial, W, with_cell, head, p.top_m);
    }
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(back, small, back_b, hipMemcpyDeviceToHost, st));
    if (volume) SLAM_HIP(hipMemcpyAsync(volume, K.volume.p, poses * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st)); // the second wait: the hits
    const int found = std::min(back[kHitCount], p.top_m);
    for (int h = 0; h < found; ++h) {
        const int32_t        *H = back + kHeadWords + kHitWords * h;
        slam_vmap_search_hit &o = hits[h];
        o.score = H[0], o.k = H[1], o.dx = H[2], o.dy = H[3], o.dz = H[4], o.n_with_cell = H[5];
        planar_k(p, o.k, (float)((double)p.cx + (double)o.dx * V.leaf), (float)((double)p.cy + (double)o.dy * V.leaf),
                 (float)((double)p.cz + (double)o.dz * V.leaf), o.init);
    }
    *n_hits = found;
    return SLAM_OK;
}

slam_vmap_search_params params_or_defaults(const slam_vmap_search_params *params)
{
    slam_vmap_search_params p;
    slam_vmap_default_search_params(&p);
    if (params) p = *params;
    return p;
}

} // namespace

extern "C" {

void slam_vmap_default_search_params(slam_vmap_search_params *p)
{
    if (!p) return;
    p->yaw0 = 0.0f, p->n_yaw = 64;
    p->cx = p->cy = p->cz = 0.0f;
    p->wx = p->wy = 24, p->wz = 0;
    p->planes_only = 1, p->min_count = 6;
    p->top_m = 4, p->nms_yaw = 2, p->nms_cells = 2;
}

int slam_vmap_search_dev(slam_vmap_t *m, const float *d_xyz, int n, int stride, const slam_vmap_search_params *params, slam_vmap_search_hit *hits,
                         int *n_hits, int32_t *volume, slam_stream_t stream)
{
    const slam_vmap_search_params p = params_or_defaults(params);
    SLAM_TRY(check_search("slam_vmap_search_dev", m, d_xyz, n, stride, p, hits, n_hits));
    SLAM_TRY(require_device());
    return search_launch("slam_vmap_search_dev", m, d_xyz, n, stride, p, hits, n_hits, volume, as_stream(stream));
}

int slam_vmap_search(slam_vmap_t *m, const float *xyz, int n, int stride, const slam_vmap_search_params *params, slam_vmap_search_hit *hits, int *n_hits,
                     int32_t *volume)
{
    const slam_vmap_search_params p = params_or_defaults(params);
    SLAM_TRY(check_search("slam_vmap_search", m, xyz, n, stride, p, hits, n_hits));
    SLAM_TRY(require_device());
    DevMem      &stage = vmap_search_work(m).stage;
    const size_t bytes = (size_t)n * stride * sizeof(float);
    if (bytes) {
        SLAM_TRY(reserve_quarter(stage, bytes));
        SLAM_HIP(hipMemcpy(stage.p, xyz, bytes, hipMemcpyHostToDevice));
    }
    return search_launch("slam_vmap_search", m, stage.as<float>(), n, stride, p, hits, n_hits, volume, nullptr);
}

int slam_vmap_search_keyframe(slam_vmap_t *m, slam_kf_t *store, int id, const slam_vmap_search_params *params, slam_vmap_search_hit *hits, int *n_hits,
                              int32_t *volume, slam_stream_t stream)
{
    const slam_vmap_search_params p = params_or_defaults(params);
    SLAM_REQUIRE(store, SLAM_E_INVALID, "slam_vmap_search_keyframe: store is NULL");
    SLAM_TRY(check_search("slam_vmap_search_keyframe", m, nullptr, 0, 4, p, hits, n_hits));
    SLAM_TRY(require_device());
    SLAM_REQUIRE(kf_live(store, id), SLAM_E_INVALID, "slam_vmap_search_keyframe: keyframe %d, the store holds %d (removed ones are refused)", id,
                 (int)store->kfs.size());
    const KfView &src = store->kfs[id].view; // the filtered cloud: float4 a point
    return search_launch("slam_vmap_search_keyframe", m, reinterpret_cast<const float *>(src.pts), src.n, 4, p, hits, n_hits, volume, as_stream(stream));
}
}
