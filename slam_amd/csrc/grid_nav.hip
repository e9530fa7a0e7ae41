// grid_nav.hip -- exact cost-to-go field from a set of goal cells over a cost plane, and the path down it
// (docs/GRID_NAV.md).  The reference has no planner: the definition is the restatement of tests/grid_nav_cases.py (a heap
// Dijkstra and whole-plane Bellman-Ford sweeps, equal to each other), and the device is held to it bit for bit.  All integer.
//
// The field is a block label-correcting relaxation.  The plane is cut into tiles of 64 x 64 cells; a ROUND is one launch with
// one workgroup of 256 per tile, and a tile whose flag is down returns at once.  A flagged tile
//   loads its potentials and cost bytes into LDS with a one-cell halo (66 x 66, the four corner cells included: a diagonal
//     move across a tile corner reads its two side cells' bytes there),
//   relaxes the tile in LDS to its local fixed point (sweeps down / up the columns, then right / left along the rows, until a
//     whole iteration changes nothing),
//   writes back the cells it owns that fell -- only the owner ever writes a cell -- and,
//   where a cell of its border fell, raises the flags of the up to eight neighbouring tiles for the NEXT round.
// A one-workgroup launch behind every round lowers the round's flags, counts, and swaps the roles of the two flag arrays.
// No workgroup waits for another: what one round needs of the one before is ordered by the stream.  A halo word read in the
// same round as its owner writes it may be the old or the new word -- both are lengths of real paths, and the owner flags the
// reader for the next round whenever it changes the word, so the fixed point is not affected.  These accesses are relaxed
// atomic loads and stores (plain instructions that pass the CU's L1), not a data race.
//
// Exactness: values only fall and every value is the length of a real path, so nothing ever lies below the true distance;
// min-plus relaxation with positive moves has one fixed point, the distance; after round k every cell whose shortest path
// crosses at most k - 1 tile borders is final: the cell where such a path last enters the tile was final a round earlier, and
// whoever wrote it flagged this tile -- its owner when the cell fell, the goals kernel when it is a goal (which never falls).  So
// the field has converged when a round raises no flag.
//
// Sums are made in 64 bits and a sum that reaches 0xFFFFFFFF is never stored: saturation, not wrap-around.  No floating
// point, and no atomic on global memory except the integer flag and counter words.
#include <memory>

#include "device_mem.hpp"
#include "grid_dist.hpp"
#include "grid_nav_table.hpp"

using namespace slam;

namespace {

constexpr int      kTile = 64;          // cells of a tile's edge (tests/grid_nav_cases.py names it: TILE)
constexpr int      kHalo = kTile + 2;   // with the one-cell halo
constexpr int      kPitch = kHalo + 1;  // 67 words a row: odd, so a wave along x and a wave along y both spread over the banks
constexpr uint32_t kFar = SLAM_GNAV_FAR;
constexpr int      kStage = 1 << 16;    // int32 pairs of the host forms' staging: goals and paths travel in pieces of this
constexpr int      kBatch = 16;         // rounds per host wait of slam_gnav_compute

struct NavState {
    slam_gnav_state s;                     // what slam_gnav_read_state hands out
    unsigned int    cur_count, next_count; // tiles flagged for the round at hand, and for the one after it
};

struct Plane {
    const uint8_t  *cost;  // [sx * sy] the handle's copy of the cost plane
    const uint32_t *S;     // [256]
    uint32_t       *pot;   // [sx * sy]
    int             sx, sy, orth_w, diag_w;
};

// A potential word that another workgroup may write or read in the same launch
__device__ __forceinline__ uint32_t pot_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pot_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// and one of the tile in LDS, which the other lanes relax at the same time
__device__ __forceinline__ uint32_t tile_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void tile_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ void flag_tile(int *flags, int t, unsigned int *count)
{
    if (atomicExch(&flags[t], 1) == 0) atomicAdd(count, 1u);
}

// every goal: valid ones get potential 0 and raise, for round 0, the flag of every tile that holds the goal cell in its tile or
// in its halo -- the cells around it, up to four tiles.  A goal never falls, so no write-back would ever tell a neighbouring tile
// to read it: a goal on a tile's border whose in-tile neighbours are closed would otherwise be seen by nobody.
__global__ __launch_bounds__(256) void gnav_goals_kernel(const int32_t *goals, int n, Plane P, int tiles_x, int *flags, NavState *st)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int x = goals[2 * i], y = goals[2 * i + 1];
        bool      ok = x >= 0 && x < P.sx && y >= 0 && y < P.sy;
        if (ok) ok = P.S[P.cost[(size_t)y * P.sx + x]] != 0;
        if (ok) {
            pot_store(&P.pot[(size_t)y * P.sx + x], 0u);
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int vx = x + dx, vy = y + dy; // (flag_tile counts a tile once however often it is named)
                    if (vx >= 0 && vx < P.sx && vy >= 0 && vy < P.sy) flag_tile(flags, (vy / kTile) * tiles_x + vx / kTile, &st->cur_count);
                }
        }
        atomicAdd((unsigned long long *)(ok ? &st->s.goals_used : &st->s.goals_skipped), 1ull);
    }
}

// behind the goals: with no valid goal nothing is flagged, everything is FAR and that is the field
__global__ void gnav_seal_kernel(NavState *st) { st->s.converged = st->cur_count == 0 ? 1 : 0; }

// One cell of the tile in LDS against its eight neighbours; true when it fell.  u = ly * kPitch + lx.
__device__ __forceinline__ bool relax_cell(uint32_t *pot, const uint8_t *cb, const uint32_t *S, int u, uint32_t ow, uint32_t dw)
{
    const uint32_t su = S[cb[u]];
    if (!su) return false; // closed: stays FAR
    const uint32_t old = tile_load(pot + u);
    uint32_t       best = old;
    // the four side cells: direction 0, 2, 4, 6
    const uint32_t s0 = S[cb[u + 1]], s2 = S[cb[u + kPitch]], s4 = S[cb[u - 1]], s6 = S[cb[u - kPitch]];
    auto           move = [&](int v, uint32_t sv, uint32_t w) {
        const uint32_t pv = tile_load(pot + v);
        if (sv && pv != kFar) {
            const unsigned long long cand = (unsigned long long)pv + (unsigned long long)(w * (su + sv)); // w (su + sv) < 2^29
            if (cand < best) best = (uint32_t)cand; // best <= FAR: a sum of 2^32 - 1 or more is never taken
        }
    };
    move(u + 1, s0, ow);
    move(u + kPitch, s2, ow);
    move(u - 1, s4, ow);
    move(u - kPitch, s6, ow);
    // a diagonal move only between two open side cells, read from this same tile (halo included)
    if (s0 && s2) move(u + kPitch + 1, S[cb[u + kPitch + 1]], dw);
    if (s4 && s2) move(u + kPitch - 1, S[cb[u + kPitch - 1]], dw);
    if (s4 && s6) move(u - kPitch - 1, S[cb[u - kPitch - 1]], dw);
    if (s0 && s6) move(u - kPitch + 1, S[cb[u - kPitch + 1]], dw);
    if (best < old) {
        tile_store(pot + u, best);
        return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void gnav_relax_kernel(Plane P, int *flags, int n_tiles, NavState *st)
{
    __shared__ uint32_t s_pot[kHalo * kPitch];
    __shared__ uint32_t s_S[kGnavTableLen];
    __shared__ uint8_t  s_cb[kHalo * kPitch];
    __shared__ unsigned s_mask;
    const int           tiles_x = gridDim.x, tile = blockIdx.y * tiles_x + blockIdx.x;
    const int           parity = (int)(st->s.rounds & 1);
    if (!flags[parity * n_tiles + tile]) return; // (uniform: the whole workgroup leaves)
    const int tid = threadIdx.x, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const int sx = P.sx, sy = P.sy;
    s_S[tid] = P.S[tid];
    if (tid == 0) s_mask = 0;
    // cells outside the plane enter as FAR with byte 0: never a source, and never a side cell of a move between plane cells
    for (int i = tid; i < kHalo * kHalo; i += 256) {
        const int ly = i / kHalo, lx = i - ly * kHalo, gx = x0 - 1 + lx, gy = y0 - 1 + ly;
        uint32_t  p = kFar;
        uint8_t   c = 0;
        if (gx >= 0 && gx < sx && gy >= 0 && gy < sy) {
            const size_t g = (size_t)gy * sx + gx;
            p = pot_load(&P.pot[g]);
            c = P.cost[g];
        }
        s_pot[ly * kPitch + lx] = p;
        s_cb[ly * kPitch + lx] = c;
    }
    __syncthreads();
    const int      nx = min(kTile, sx - x0), ny = min(kTile, sy - y0); // the plane's cells of this tile
    const int      lane = tid & 63, strip = tid >> 6;
    const uint32_t ow = (uint32_t)P.orth_w, dw = (uint32_t)P.diag_w;
    // To the local fixed point.  An iteration in which no cell fell has checked every cell against values that did not move.
    for (;;) {
        int changed = 0;
        if (lane < nx) { // lanes along x, each down and up a strip of 16 rows
            const int lx = 1 + lane, r0 = 1 + 16 * strip, r1 = min(r0 + 16, ny + 1);
            for (int ly = r0; ly < r1; ++ly) changed |= relax_cell(s_pot, s_cb, s_S, ly * kPitch + lx, ow, dw);
            for (int ly = r1 - 1; ly >= r0; --ly) changed |= relax_cell(s_pot, s_cb, s_S, ly * kPitch + lx, ow, dw);
        }
        __syncthreads();
        if (lane < ny) { // lanes along y, each right and left along a strip of 16 columns
            const int ly = 1 + lane, c0 = 1 + 16 * strip, c1 = min(c0 + 16, nx + 1);
            for (int lx = c0; lx < c1; ++lx) changed |= relax_cell(s_pot, s_cb, s_S, ly * kPitch + lx, ow, dw);
            for (int lx = c1 - 1; lx >= c0; --lx) changed |= relax_cell(s_pot, s_cb, s_S, ly * kPitch + lx, ow, dw);
        }
        if (!__syncthreads_or(changed)) break;
    }
    // the owner's write-back, and which neighbours read a cell that fell:
    // bit 0 west, 1 east, 2 north (y - 1), 3 south, 4 north-west, 5 north-east, 6 south-west, 7 south-east
    unsigned mask = 0;
    for (int i = tid; i < kTile * kTile; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        if (lx >= nx || ly >= ny) continue;
        const size_t   g = (size_t)(y0 + ly) * sx + (x0 + lx);
        const uint32_t v = s_pot[(ly + 1) * kPitch + lx + 1];
        if (v < pot_load(&P.pot[g])) {
            pot_store(&P.pot[g], v);
            const bool w = lx == 0, e = lx == kTile - 1, n = ly == 0, s = ly == kTile - 1;
            mask |= (w ? 1u : 0) | (e ? 2u : 0) | (n ? 4u : 0) | (s ? 8u : 0) | (n && w ? 16u : 0) | (n && e ? 32u : 0) | (s && w ? 64u : 0) |
                    (s && e ? 128u : 0);
        }
    }
    if (mask) atomicOr(&s_mask, mask);
    __syncthreads();
    if (tid < 8 && (s_mask >> tid & 1)) {
        const int dx = tid == 0 || tid == 4 || tid == 6 ? -1 : (tid == 1 || tid == 5 || tid == 7 ? 1 : 0);
        const int dy = tid == 2 || tid == 4 || tid == 5 ? -1 : (tid == 3 || tid == 6 || tid == 7 ? 1 : 0);
        const int tx = (int)blockIdx.x + dx, ty = (int)blockIdx.y + dy;
        if (tx >= 0 && tx < tiles_x && ty >= 0 && ty < (int)gridDim.y) flag_tile(flags + (1 - parity) * n_tiles, ty * tiles_x + tx, &st->next_count);
    }
}

// behind every round: the round's flags go down, the counts move on, the two flag arrays change roles
__global__ __launch_bounds__(256) void gnav_advance_kernel(int *flags, int n_tiles, NavState *st)
{
    int *cur = flags + (st->s.rounds & 1) * n_tiles;
    for (int i = threadIdx.x; i < n_tiles; i += 256) cur[i] = 0;
    __syncthreads(); // (every thread has read the parity)
    if (threadIdx.x == 0) {
        st->s.tiles_processed += st->cur_count;
        st->s.rounds += 1;
        st->s.converged = st->next_count == 0 ? 1 : 0;
        st->cur_count = st->next_count;
        st->next_count = 0;
    }
}

// direction d = 0..7: (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1)
__device__ __forceinline__ int dir_dx(int d) { return (d <= 1 || d == 7 ? 1 : 0) - (d >= 3 && d <= 5 ? 1 : 0); }
__device__ __forceinline__ int dir_dy(int d) { return (d >= 1 && d <= 3 ? 1 : 0) - (d >= 5 ? 1 : 0); }

// One wave.  Lanes 0..7 look at the eight neighbours; the lowest direction whose potential plus the move equals this cell's
// is the next cell.  Every step lowers the potential, and the walk ends at max_len whatever the field holds.
__global__ __launch_bounds__(64) void gnav_path_kernel(Plane P, int x, int y, int max_len, int prior, int32_t *path, int32_t *len_status,
                                                       NavState *st)
{
    const int lane = threadIdx.x;
    int       len = 0, status = SLAM_GNAV_PATH_NOT_CONVERGED;
    if (st->s.converged) {
        const bool inside = x >= 0 && x < P.sx && y >= 0 && y < P.sy;
        uint32_t   su = inside ? P.S[P.cost[(size_t)y * P.sx + x]] : 0u;
        uint32_t   pu = su ? P.pot[(size_t)y * P.sx + x] : kFar;
        status = pu == kFar ? SLAM_GNAV_PATH_NO_START : SLAM_GNAV_PATH_CUT;
        while (status == SLAM_GNAV_PATH_CUT && len < max_len) {
            if (lane == 0) path[2 * len] = x, path[2 * len + 1] = y;
            ++len;
            if (pu == 0) { // only a goal has potential 0: every move costs at least 2
                status = SLAM_GNAV_PATH_REACHED;
                break;
            }
            if (len == max_len) break;
            bool     ok = false;
            uint32_t pv = kFar, sv = 0;
            if (lane < 8) {
                const int dx = dir_dx(lane), dy = dir_dy(lane), vx = x + dx, vy = y + dy;
                if (vx >= 0 && vx < P.sx && vy >= 0 && vy < P.sy) {
                    sv = P.S[P.cost[(size_t)vy * P.sx + vx]];
                    pv = P.pot[(size_t)vy * P.sx + vx];
                    bool allowed = sv != 0 && pv != kFar;
                    if (allowed && dx != 0 && dy != 0) // the two side cells lie inside the plane when u and v do
                        allowed = P.S[P.cost[(size_t)y * P.sx + vx]] != 0 && P.S[P.cost[(size_t)vy * P.sx + x]] != 0;
                    const uint32_t w = (uint32_t)(dx != 0 && dy != 0 ? P.diag_w : P.orth_w);
                    ok = allowed && (unsigned long long)pv + (unsigned long long)(w * (su + sv)) == (unsigned long long)pu;
                }
            }
            const unsigned long long found = __ballot(ok);
            if (!found) { // not on an exact field; the caller's plane was not the one the field was computed on
                status = SLAM_GNAV_PATH_NOT_CONVERGED;
                len = 0;
                break;
            }
            const int d = __ffsll((long long)found) - 1;
            x += dir_dx(d);
            y += dir_dy(d);
            pu = (uint32_t)__shfl((int)pv, d);
            su = (uint32_t)__shfl((int)sv, d);
        }
    }
    if (lane == 0) {
        len_status[0] = len;
        len_status[1] = status;
        st->s.last_path_len = (status == SLAM_GNAV_PATH_REACHED || status == SLAM_GNAV_PATH_CUT) ? prior + len : 0;
        st->s.last_path_status = status;
    }
}

} // namespace

struct slam_gnav {
    int    sx = 0, sy = 0, orth_w = 0, diag_w = 0, tiles_x = 0, tiles_y = 0, n_tiles = 0;
    size_t cells = 0;
    bool   started = false; // a restart has been enqueued: there is a field to continue, read and walk
    OwnedArray<uint32_t> d_pot;   // [cells]
    OwnedArray<uint8_t>  d_cost;  // [cells] the plane of the last restart
    OwnedArray<uint32_t> d_table; // [256]
    OwnedArray<int>      d_flags; // [2][n_tiles]
    OwnedArray<NavState> d_state;
    OwnedArray<int32_t>  d_stage; // [2 * kStage + 2] the host forms' goals and path pieces, then (length, status)
    OwnedArray<long long, Mem::Pinned> h_word; // what slam_gnav_compute reads per batch

    Plane plane() const { return Plane{d_cost.get(), d_table.get(), d_pot.get(), sx, sy, orth_w, diag_w}; }
};

namespace {

// the field starts over on a copy of d_cost: FAR everywhere, flags and state zero
int enqueue_restart(slam_gnav *h, const uint8_t *d_cost, hipStream_t st)
{
    if (d_cost != h->d_cost.get()) SLAM_HIP(hipMemcpyAsync(h->d_cost.get(), d_cost, h->cells, hipMemcpyDeviceToDevice, st));
    SLAM_HIP(hipMemsetAsync(h->d_pot.get(), 0xFF, h->cells * sizeof(uint32_t), st));
    SLAM_HIP(hipMemsetAsync(h->d_flags.get(), 0, sizeof(int) * 2 * (size_t)h->n_tiles, st));
    SLAM_HIP(hipMemsetAsync(h->d_state.get(), 0, sizeof(NavState), st));
    h->started = true;
    return SLAM_OK;
}

int enqueue_goals(slam_gnav *h, const int32_t *d_goals, int n, hipStream_t st)
{
    hipLaunchKernelGGL(gnav_goals_kernel, dim3(std::min((n + 255) / 256, 1024)), dim3(256), 0, st, d_goals, n, h->plane(), h->tiles_x,
                       h->d_flags.get(), h->d_state.get());
    return SLAM_OK;
}

int enqueue_rounds(slam_gnav *h, int rounds, hipStream_t st)
{
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(gnav_relax_kernel, dim3(h->tiles_x, h->tiles_y), dim3(256), 0, st, h->plane(), h->d_flags.get(), h->n_tiles,
                           h->d_state.get());
        hipLaunchKernelGGL(gnav_advance_kernel, dim3(1), dim3(256), 0, st, h->d_flags.get(), h->n_tiles, h->d_state.get());
    }
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int compute_on(slam_gnav *h, const uint8_t *d_cost, const int32_t *d_goals, int n_goals, int rounds, int restart, hipStream_t st)
{
    if (restart) {
        SLAM_TRY(enqueue_restart(h, d_cost, st));
        SLAM_TRY(enqueue_goals(h, d_goals, n_goals, st));
        hipLaunchKernelGGL(gnav_seal_kernel, dim3(1), dim3(1), 0, st, h->d_state.get());
    }
    return enqueue_rounds(h, rounds, st);
}

} // namespace

extern "C" {

void slam_gnav_default_params(slam_gnav_params *p)
{
    if (!p) return;
    p->orth_w = 12, p->diag_w = 17; // within 0.2 % of 1 : sqrt 2
    p->neutral = 50, p->lethal_from = 253, p->unknown_step = 0; // 253: costmap_2d INSCRIBED_INFLATED_OBSTACLE
}

int slam_grid_step_table(int neutral, int lethal_from, int unknown_step, uint32_t *table, int n)
{
    const char *why = "";
    if (grid_step_table(neutral, lethal_from, unknown_step, table, n, &why) != 0) {
        set_error("slam_grid_step_table: %s", why);
        return SLAM_E_INVALID;
    }
    return SLAM_OK;
}

int slam_gnav_create(int size_x, int size_y, const slam_gnav_params *params, slam_gnav_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_gnav_create: null out pointer");
    *out = nullptr;
    slam_gnav_params p;
    slam_gnav_default_params(&p);
    if (params) p = *params;
    SLAM_REQUIRE(size_x > 0 && size_y > 0 && size_x <= 32767 && size_y <= 32767, SLAM_E_INVALID, "slam_gnav_create: size must be 1..32767 cells");
    SLAM_REQUIRE(p.orth_w >= 1 && p.orth_w <= kGnavMaxWeight && p.diag_w >= 1 && p.diag_w <= kGnavMaxWeight, SLAM_E_INVALID,
                 "slam_gnav_create: orth_w and diag_w must be 1..255");
    uint32_t    table[kGnavTableLen];
    const char *why = "";
    SLAM_REQUIRE(grid_step_table(p.neutral, p.lethal_from, p.unknown_step, table, kGnavTableLen, &why) == 0, SLAM_E_INVALID,
                 "slam_gnav_create: %s", why);
    SLAM_TRY(require_device());
    std::unique_ptr<slam_gnav> h(new (std::nothrow) slam_gnav());
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_gnav_create: out of host memory");
    h->sx = size_x, h->sy = size_y, h->orth_w = p.orth_w, h->diag_w = p.diag_w;
    h->tiles_x = (size_x + kTile - 1) / kTile, h->tiles_y = (size_y + kTile - 1) / kTile;
    h->n_tiles = h->tiles_x * h->tiles_y;
    h->cells = (size_t)size_x * size_y;
    SLAM_TRY(h->d_pot.alloc(h->cells * sizeof(uint32_t)));
    SLAM_TRY(h->d_cost.alloc(h->cells));
    SLAM_TRY(h->d_table.alloc(sizeof(uint32_t) * kGnavTableLen));
    SLAM_TRY(h->d_flags.alloc(sizeof(int) * 2 * (size_t)h->n_tiles));
    SLAM_TRY(h->d_state.alloc(sizeof(NavState)));
    SLAM_TRY(h->d_stage.alloc(sizeof(int32_t) * (2 * (size_t)kStage + 2)));
    SLAM_TRY(h->h_word.alloc(sizeof(long long)));
    SLAM_HIP(hipMemcpy(h->d_table.get(), table, sizeof(table), hipMemcpyHostToDevice));
    SLAM_HIP(hipMemset(h->d_state.get(), 0, sizeof(NavState)));
    *out = h.release();
    return SLAM_OK;
}

void slam_gnav_destroy(slam_gnav_t *h) { delete h; } // (the frees wait for the device)

int slam_gnav_set_table(slam_gnav_t *h, const uint32_t *table, int n)
{
    SLAM_REQUIRE(h && table, SLAM_E_INVALID, "slam_gnav_set_table: bad arguments");
    SLAM_REQUIRE(n == kGnavTableLen, SLAM_E_INVALID, "slam_gnav_set_table: the table has 256 entries, not %d", n);
    SLAM_REQUIRE(grid_step_table_ok(table, n), SLAM_E_INVALID, "slam_gnav_set_table: an entry above 2^20");
    SLAM_HIP(hipDeviceSynchronize()); // a compute still in flight reads the old table
    SLAM_HIP(hipMemcpy(h->d_table.get(), table, sizeof(uint32_t) * kGnavTableLen, hipMemcpyHostToDevice));
    return SLAM_OK;
}

int slam_gnav_compute_dev(slam_gnav_t *h, const uint8_t *d_cost, const int32_t *d_goals, int n_goals, int rounds, int restart,
                          slam_stream_t stream)
{
    SLAM_REQUIRE(h && d_cost && d_goals, SLAM_E_INVALID, "slam_gnav_compute_dev: null pointer");
    SLAM_REQUIRE(n_goals >= 1, SLAM_E_INVALID, "slam_gnav_compute_dev: n_goals must be at least 1");
    SLAM_REQUIRE(rounds >= 0, SLAM_E_INVALID, "slam_gnav_compute_dev: rounds must not be negative");
    SLAM_REQUIRE(restart || h->started, SLAM_E_INVALID, "slam_gnav_compute_dev: nothing to continue (no restart yet)");
    return compute_on(h, d_cost, d_goals, n_goals, rounds, restart, as_stream(stream));
}

int slam_gnav_compute(slam_gnav_t *h, const uint8_t *cost, const int32_t *goals, int n_goals, int max_rounds)
{
    SLAM_REQUIRE(h && cost && goals, SLAM_E_INVALID, "slam_gnav_compute: null pointer");
    SLAM_REQUIRE(n_goals >= 1, SLAM_E_INVALID, "slam_gnav_compute: n_goals must be at least 1");
    SLAM_REQUIRE(max_rounds >= 0, SLAM_E_INVALID, "slam_gnav_compute: max_rounds must not be negative");
    SLAM_HIP(hipMemcpy(h->d_cost.get(), cost, h->cells, hipMemcpyHostToDevice));
    SLAM_TRY(enqueue_restart(h, h->d_cost.get(), nullptr));
    for (int off = 0; off < n_goals; off += kStage) { // (each copy waits for the piece before it)
        const int n = std::min(kStage, n_goals - off);
        SLAM_HIP(hipMemcpy(h->d_stage.get(), goals + 2 * (size_t)off, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice));
        SLAM_TRY(enqueue_goals(h, h->d_stage.get(), n, nullptr));
    }
    hipLaunchKernelGGL(gnav_seal_kernel, dim3(1), dim3(1), 0, nullptr, h->d_state.get());
    // After round k every cell whose shortest path crosses at most k - 1 tile borders is final, and a shortest path visits no
    // cell twice: cells + 1 rounds always suffice, so the loop ends.
    const long long limit = max_rounds ? (long long)max_rounds : (long long)h->cells + 1;
    *h->h_word.get() = 0;
    for (long long done = 0; done < limit;) {
        const int b = (int)std::min<long long>(kBatch, limit - done);
        SLAM_TRY(enqueue_rounds(h, b, nullptr));
        SLAM_HIP(hipMemcpyAsync(h->h_word.get(), &h->d_state.get()->s.converged, sizeof(long long), hipMemcpyDeviceToHost, nullptr));
        SLAM_HIP(hipStreamSynchronize(nullptr));
        done += b;
        if (*h->h_word.get()) return SLAM_OK;
    }
    set_error("slam_gnav_compute: not converged after %lld rounds", limit);
    return SLAM_E_TIMEOUT;
}

int slam_gnav_read(slam_gnav_t *h, uint32_t *pot)
{
    SLAM_REQUIRE(h && pot, SLAM_E_INVALID, "slam_gnav_read: bad arguments");
    SLAM_REQUIRE(h->started, SLAM_E_INVALID, "slam_gnav_read: nothing has been computed");
    SLAM_HIP(hipDeviceSynchronize()); // whichever stream the last compute went to
    SLAM_HIP(hipMemcpy(pot, h->d_pot.get(), h->cells * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_gnav_potential_dev(slam_gnav_t *h, uint32_t **d_pot)
{
    SLAM_REQUIRE(h && d_pot, SLAM_E_INVALID, "slam_gnav_potential_dev: bad arguments");
    *d_pot = h->d_pot.get();
    return SLAM_OK;
}

int slam_gnav_path_dev(slam_gnav_t *h, int sx, int sy, int max_len, int32_t *d_path, int32_t *d_len_status, slam_stream_t stream)
{
    SLAM_REQUIRE(h && d_path && d_len_status, SLAM_E_INVALID, "slam_gnav_path_dev: null pointer");
    SLAM_REQUIRE(max_len >= 1, SLAM_E_INVALID, "slam_gnav_path_dev: max_len must be at least 1");
    SLAM_REQUIRE(h->started, SLAM_E_INVALID, "slam_gnav_path_dev: nothing has been computed");
    hipLaunchKernelGGL(gnav_path_kernel, dim3(1), dim3(64), 0, as_stream(stream), h->plane(), sx, sy, max_len, 0, d_path, d_len_status,
                       h->d_state.get());
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_gnav_path(slam_gnav_t *h, int sx, int sy, int max_len, int32_t *path, int *len, int *status)
{
    SLAM_REQUIRE(h && path && len && status, SLAM_E_INVALID, "slam_gnav_path: null pointer");
    SLAM_REQUIRE(max_len >= 1, SLAM_E_INVALID, "slam_gnav_path: max_len must be at least 1");
    SLAM_REQUIRE(h->started, SLAM_E_INVALID, "slam_gnav_path: nothing has been computed");
    SLAM_HIP(hipDeviceSynchronize()); // whichever stream the last compute went to
    // In pieces of at most kStage cells through the staging block; a piece that was cut before max_len is continued from its
    // last cell, which the next piece writes again.
    int32_t *d_piece = h->d_stage.get(), *d_ls = d_piece + 2 * (size_t)kStage;
    int      total = 0, x = sx, y = sy, st = SLAM_GNAV_PATH_CUT;
    for (;;) {
        const int prior = total ? total - 1 : 0, n = std::min(max_len - prior, kStage);
        int32_t   ls[2];
        hipLaunchKernelGGL(gnav_path_kernel, dim3(1), dim3(64), 0, nullptr, h->plane(), x, y, n, prior, d_piece, d_ls, h->d_state.get());
        SLAM_HIP(hipGetLastError());
        SLAM_HIP(hipMemcpy(ls, d_ls, sizeof(ls), hipMemcpyDeviceToHost));
        if (ls[0] > 0) SLAM_HIP(hipMemcpy(path + 2 * (size_t)prior, d_piece, sizeof(int32_t) * 2 * (size_t)ls[0], hipMemcpyDeviceToHost));
        st = ls[1];
        if (st == SLAM_GNAV_PATH_NO_START || st == SLAM_GNAV_PATH_NOT_CONVERGED) {
            total = 0;
            break;
        }
        total = prior + ls[0];
        if (st == SLAM_GNAV_PATH_REACHED || total >= max_len) break;
        x = path[2 * (size_t)(total - 1)], y = path[2 * (size_t)(total - 1) + 1];
    }
    *len = total;
    *status = st;
    return SLAM_OK;
}

int slam_gnav_read_state(slam_gnav_t *h, slam_gnav_state *state)
{
    SLAM_REQUIRE(h && state, SLAM_E_INVALID, "slam_gnav_read_state: bad arguments");
    SLAM_HIP(hipDeviceSynchronize());
    SLAM_HIP(hipMemcpy(state, &h->d_state.get()->s, sizeof(*state), hipMemcpyDeviceToHost)); // the record's first member
    return SLAM_OK;
}

int slam_grid_nav_field(slam_grid_t *g, slam_gdist_t *gdist, slam_gnav_t *gnav, const int32_t *d_goals, int n_goals, int rounds,
                        slam_stream_t stream)
{
    SLAM_REQUIRE(g && gdist && gnav && d_goals, SLAM_E_INVALID, "slam_grid_nav_field: null pointer");
    SLAM_REQUIRE(n_goals >= 1, SLAM_E_INVALID, "slam_grid_nav_field: n_goals must be at least 1");
    SLAM_REQUIRE(rounds >= 0, SLAM_E_INVALID, "slam_grid_nav_field: rounds must not be negative");
    int gx = 0, gy = 0, dx = 0, dy = 0;
    SLAM_TRY(slam_grid_info(g, &gx, &gy, nullptr, nullptr, nullptr));
    gdist_size(gdist, &dx, &dy);
    SLAM_REQUIRE(gx == gnav->sx && gy == gnav->sy && dx == gnav->sx && dy == gnav->sy, SLAM_E_INVALID,
                 "slam_grid_nav_field: the grid is %d x %d cells, the distance field %d x %d, the navigation field %d x %d", gx, gy, dx, dy,
                 gnav->sx, gnav->sy);
    uint8_t *d_cost = nullptr;
    SLAM_TRY(slam_gdist_planes_dev(gdist, nullptr, &d_cost));
    SLAM_REQUIRE(d_cost, SLAM_E_INVALID, "slam_grid_nav_field: the distance field has no table, so no cost plane (slam_gdist_set_table)");
    return compute_on(gnav, d_cost, d_goals, n_goals, rounds, 1, as_stream(stream));
}

} // extern "C"
