// kf_sc.hip -- appearance-based loop-closure candidates for the keyframe store (slam_kf_sc_*, docs/SCAN_CONTEXT.md): a
// polar height descriptor per keyframe in the spirit of Scan Context (Kim & Kim, IROS 2018) and an exhaustive, exact
// search over all keyframes and all yaw shifts.  A point is binned by comparisons of correctly rounded f64 products (no
// sqrt, no atan2) against tables the host made; everything behind the binning is integer, so the result does not depend
// on the order of points or threads and equals the scalar restatement (tests/cpp/sc_oracle.cpp) bit for bit.
#include <climits>

#include "kf_common.hpp"

namespace {

constexpr int kScThreads = 256;
constexpr int kScMaxRings = 32, kScMaxSectors = 128;

struct ScTables { // a kernel argument: the loops below index it uniformly
    double edge2[kScMaxRings];      // (k + 1)^2 (max_range / n_rings)^2
    double c[kScMaxSectors / 4], s[kScMaxSectors / 4]; // cos, sin(2 pi k / n_sectors); entry 0 unused
    double z_min, inv_step;
    int    n_rings, n_sectors;
};

struct ScTask {
    const float4 *pts;
    uint32_t     *desc; // n_rings * n_sectors bytes, written four to a word
    int           n, pad;
};

// The cell and the height code of a point; false = dropped.
__device__ inline bool sc_cell(const ScTables &T, float x, float y, float z, int *cell, uint32_t *h)
{
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    const double r2 = __dadd_rn(__dmul_rn((double)x, (double)x), __dmul_rn((double)y, (double)y));
    int          ring = 0;
    for (int k = 0; k < T.n_rings; ++k) ring += T.edge2[k] <= r2 ? 1 : 0;
    if (ring >= T.n_rings) return false;
    int   q;
    float px, py;
    if (x > 0.0f && y >= 0.0f)
        q = 0, px = x, py = y;
    else if (x <= 0.0f && y > 0.0f)
        q = 1, px = y, py = -x;
    else if (x < 0.0f && y <= 0.0f)
        q = 2, px = -x, py = -y;
    else if (x >= 0.0f && y < 0.0f)
        q = 3, px = -y, py = x;
    else // the origin
        q = 0, px = 1.0f, py = 0.0f;
    const int per = T.n_sectors >> 2;
    int       j = 0;
    // two products, each rounded, then compared: never a difference of products
    for (int k = 1; k < per; ++k) j += __dmul_rn((double)py, T.c[k]) >= __dmul_rn((double)px, T.s[k]) ? 1 : 0;
    double f = floor(__dmul_rn(__dsub_rn((double)z, T.z_min), T.inv_step));
    f = f < 0.0 ? 0.0 : f > 254.0 ? 254.0 : f;
    *cell = ring * T.n_sectors + q * per + j;
    *h = 1u + (uint32_t)(int)f;
    return true;
}

// One workgroup per keyframe.  The cells sit in LDS as u32 under atomicMax, which is order-free; packed to bytes at the end.
__global__ __launch_bounds__(kScThreads) void kf_sc_desc_kernel(const ScTask *tasks, ScTables T)
{
    __shared__ uint32_t cells[kScMaxRings * kScMaxSectors];
    const ScTask        t = tasks[blockIdx.x];
    const int           nc = T.n_rings * T.n_sectors, tid = threadIdx.x;
    for (int i = tid; i < nc; i += kScThreads) cells[i] = 0u;
    __syncthreads();
    for (int i = tid; i < t.n; i += kScThreads) {
        const float4 p = t.pts[i];
        int          cell;
        uint32_t     h;
        if (sc_cell(T, p.x, p.y, p.z, &cell, &h)) atomicMax(&cells[cell], h);
    }
    __syncthreads();
    for (int w = tid; w < (nc >> 2); w += kScThreads) // n_sectors is a multiple of 4
        t.desc[w] = cells[4 * w] | (cells[4 * w + 1] << 8) | (cells[4 * w + 2] << 16) | (cells[4 * w + 3] << 24);
}

// ---------------------------------------------------------------- the search
// four bytes starting `sh` / 8 bytes into the little-endian pair (lo, hi)
__device__ inline uint32_t bytes_at(uint32_t lo, uint32_t hi, int sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh); }

__device__ inline uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc)
{
#if __has_builtin(__builtin_amdgcn_sad_u8)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int k = 0; k < 4; ++k) {
        const int x = (int)((a >> (8 * k)) & 255u), y = (int)((b >> (8 * k)) & 255u);
        acc += (uint32_t)(x > y ? x - y : y - x);
    }
    return acc;
#endif
}

// bit 7 of every byte of x that is not zero
__device__ inline uint32_t occupied4(uint32_t x) { return (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u; }

// One workgroup per (query, candidate) pair: a query against N keyframes is N workgroups, which fills the device already
// for the on-line case of one query.  Both descriptors sit in LDS as words of four cells; the candidate's rows are stored
// twice over (and one word more), so that shift s is the byte offset n_sectors - s into the row and not a modulo.  Thread
// t owns shift t % S and the rings t / S, t / S + G, ... (G = 256 / S groups); lanes next to each other read the same or
// the next word of a row (a broadcast, no bank conflict).  The groups' partial sums are added per shift in the order of the
// groups, then the argmin over shifts is a minimum of the keys (D << 8) | s.  Integers throughout.
__global__ __launch_bounds__(kScThreads) void kf_sc_match_kernel(const uint8_t *const *desc, const int *queries, slam_kf_sc_match_t *out, int count,
                                                                 int R, int S)
{
    __shared__ uint32_t sa[kScMaxRings * (kScMaxSectors / 4)];
    __shared__ uint32_t sb[kScMaxRings * (kScMaxSectors / 2 + 1)];
    __shared__ uint32_t part[kScThreads];
    __shared__ uint32_t wkey[kScThreads / 64];
    __shared__ int      wcnt[kScThreads / 64][3];
    const int           tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int           qid = queries[blockIdx.x / (unsigned)count], id = (int)(blockIdx.x % (unsigned)count);
    const uint8_t      *a = desc[qid], *b = desc[id];
    slam_kf_sc_match_t *o = out + blockIdx.x;
    if (!b || id == qid) { // the whole workgroup alike
        if (tid == 0) o->distance = -1, o->shift = 0, o->n_query = 0, o->n_candidate = 0, o->n_both = 0;
        return;
    }
    const int       W = S >> 2, BW = 2 * W + 1;
    const uint32_t *aw = reinterpret_cast<const uint32_t *>(a), *bw = reinterpret_cast<const uint32_t *>(b);
    for (int i = tid; i < R * W; i += kScThreads) sa[i] = aw[i];
    for (int i = tid; i < R * BW; i += kScThreads) {
        const int r = i / BW, j = i - r * BW;
        sb[i] = bw[r * W + j % W];
    }
    __syncthreads();
    const int G = kScThreads / S, s = tid % S, g = tid / S;
    if (g < G) {
        const int off = S - s, ow = off >> 2, sh = (off & 3) * 8;
        uint32_t  d = 0u;
        for (int r = g; r < R; r += G) {
            const uint32_t *ar = sa + r * W, *br = sb + r * BW + ow;
            uint32_t        lo = br[0];
            for (int w = 0; w < W; ++w) {
                const uint32_t hi = br[w + 1];
                d = sad4(ar[w], bytes_at(lo, hi, sh), d);
                lo = hi;
            }
        }
        part[tid] = d;
    }
    __syncthreads();
    uint32_t key = ~0u;
    if (tid < S) {
        uint32_t D = 0u;
        for (int k = 0; k < G; ++k) D += part[k * S + tid];
        key = (D << 8) | (uint32_t)tid; // D <= 255 * 32 * 128 < 2^20, tid < 128
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t other = __shfl_down(key, d, 64);
        key = other < key ? other : key;
    }
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    key = wkey[0];
    for (int w = 1; w < kScThreads / 64; ++w) key = wkey[w] < key ? wkey[w] : key;
    // the occupied cells at the best shift
    const int best = (int)(key & 255u), off = S - best, ow = off >> 2, sh = (off & 3) * 8;
    int       cnt[3] = {0, 0, 0};
    for (int i = tid; i < R * W; i += kScThreads) {
        const int       r = i / W, w = i - r * W;
        const uint32_t *br = sb + r * BW + ow + w;
        const uint32_t  ma = occupied4(sa[i]), mb = occupied4(bytes_at(br[0], br[1], sh));
        cnt[0] += __popc(ma), cnt[1] += __popc(mb), cnt[2] += __popc(ma & mb);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int x = cnt[k];
        for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
        if (lane == 0) wcnt[wave][k] = x;
    }
    __syncthreads();
    if (tid == 0) {
        int tot[3] = {0, 0, 0};
        for (int w = 0; w < kScThreads / 64; ++w)
            for (int k = 0; k < 3; ++k) tot[k] += wcnt[w][k];
        o->distance = (int)(key >> 8), o->shift = best, o->n_query = tot[0], o->n_candidate = tot[1], o->n_both = tot[2];
    }
}

int check_sc_params(const slam_kf_sc_params *p)
{
    SLAM_REQUIRE(p->n_rings >= 1 && p->n_rings <= kScMaxRings, SLAM_E_INVALID, "slam_kf_set_sc_params: n_rings %d is not in 1 .. %d", p->n_rings,
                 kScMaxRings);
    SLAM_REQUIRE(p->n_sectors >= 4 && p->n_sectors <= kScMaxSectors && p->n_sectors % 4 == 0, SLAM_E_INVALID,
                 "slam_kf_set_sc_params: n_sectors %d is not a multiple of 4 in 4 .. %d", p->n_sectors, kScMaxSectors);
    SLAM_REQUIRE(std::isfinite(p->max_range) && p->max_range > 0.0, SLAM_E_INVALID, "slam_kf_set_sc_params: max_range %g is not positive", p->max_range);
    SLAM_REQUIRE(std::isfinite(p->z_step) && p->z_step > 0.0 && std::isfinite(1.0 / p->z_step), SLAM_E_INVALID,
                 "slam_kf_set_sc_params: z_step %g is not positive", p->z_step);
    SLAM_REQUIRE(std::isfinite(p->z_min), SLAM_E_INVALID, "slam_kf_set_sc_params: z_min %g is not finite", p->z_min);
    return SLAM_OK;
}

void sc_make_tables(slam_kf *s)
{
    if (s->sc_tables_ready) return;
    const slam_kf_sc_params &p = s->sp;
    for (int k = 0; k < kScMaxRings; ++k) {
        const double e = (k + 1) * (p.max_range / p.n_rings);
        s->sc_edge2[k] = e * e;
        s->sc_cos[k] = cos(2.0 * M_PI * k / p.n_sectors);
        s->sc_sin[k] = sin(2.0 * M_PI * k / p.n_sectors);
    }
    s->sc_tables_ready = true;
}

} // namespace

extern "C" {

void slam_kf_sc_default_params(slam_kf_sc_params *p)
{
    if (!p) return;
    p->n_rings = 20, p->n_sectors = 64; // Scan Context's 20 x 60, the sectors rounded up to whole words
    p->max_range = 80.0;
    p->z_min = -2.0, p->z_step = 0.02; // 254 bins of 2 cm: 5.08 m above z_min
}

int slam_kf_set_sc_params(slam_kf_t *s, const slam_kf_sc_params *params)
{
    SLAM_REQUIRE(s && params, SLAM_E_INVALID, "slam_kf_set_sc_params: null argument");
    SLAM_TRY(check_sc_params(params));
    SLAM_REQUIRE(s->n_sc == 0 || (params->n_rings == s->sp.n_rings && params->n_sectors == s->sp.n_sectors && params->max_range == s->sp.max_range &&
                                  params->z_min == s->sp.z_min && params->z_step == s->sp.z_step),
                 SLAM_E_INVALID, "slam_kf_set_sc_params: the parameters are fixed once a keyframe holds a descriptor");
    s->sp = *params;
    s->sc_tables_ready = false;
    return SLAM_OK;
}

int slam_kf_sc_read_tables(slam_kf_t *s, double *edge2, double *c, double *sn)
{
    SLAM_REQUIRE(s && edge2 && c && sn, SLAM_E_INVALID, "slam_kf_sc_read_tables: null argument");
    sc_make_tables(s);
    std::memcpy(edge2, s->sc_edge2, sizeof(double) * s->sp.n_rings);
    std::memcpy(c, s->sc_cos, sizeof(double) * (s->sp.n_sectors / 4));
    std::memcpy(sn, s->sc_sin, sizeof(double) * (s->sp.n_sectors / 4));
    return SLAM_OK;
}

int slam_kf_sc_compute(slam_kf_t *s, int id, slam_stream_t stream)
{
    SLAM_REQUIRE(s && (id == -1 || kf_live(s, id)), SLAM_E_INVALID, "slam_kf_sc_compute: no keyframe %d", id);
    const int first = id < 0 ? 0 : id, last = id < 0 ? (int)s->kfs.size() : id + 1;
    int       n = 0;
    for (int k = first; k < last; ++k) n += !s->kfs[k].removed && !s->kfs[k].sc.p ? 1 : 0;
    if (n == 0) return SLAM_OK;
    sc_make_tables(s);
    const size_t        desc_b = (size_t)s->sp.n_rings * s->sp.n_sectors;
    std::vector<DevMem> fresh(n); // handed to the keyframes once the launch has succeeded
    for (DevMem &m : fresh) SLAM_TRY(m.alloc(desc_b));
    SLAM_TRY(reserve_quarter(s->work, sizeof(ScTask) * (size_t)n));
    ScTask *tasks = static_cast<ScTask *>(pinned_scratch(sizeof(ScTask) * (size_t)n));
    SLAM_REQUIRE(tasks, SLAM_E_NOMEM, "slam_kf_sc_compute: no pinned staging memory");
    int e = 0;
    for (int k = first; k < last; ++k) {
        const Keyframe &kf = s->kfs[k];
        if (kf.removed || kf.sc.p) continue;
        tasks[e].pts = kf.view.pts, tasks[e].n = kf.view.n, tasks[e].pad = 0;
        tasks[e].desc = fresh[e].as<uint32_t>();
        ++e;
    }
    ScTables T;
    std::memcpy(T.edge2, s->sc_edge2, sizeof T.edge2);
    std::memcpy(T.c, s->sc_cos, sizeof T.c);
    std::memcpy(T.s, s->sc_sin, sizeof T.s);
    T.z_min = s->sp.z_min, T.inv_step = 1.0 / s->sp.z_step;
    T.n_rings = s->sp.n_rings, T.n_sectors = s->sp.n_sectors;
    hipStream_t st = as_stream(stream);
    SLAM_HIP(hipMemcpyAsync(s->work.p, tasks, sizeof(ScTask) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kf_sc_desc_kernel, dim3(n), dim3(kScThreads), 0, st, s->work.as<const ScTask>(), T);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipStreamSynchronize(st));
    e = 0;
    for (int k = first; k < last; ++k) {
        Keyframe &kf = s->kfs[k];
        if (kf.removed || kf.sc.p) continue;
        kf.sc = std::move(fresh[e++]);
    }
    s->n_sc += n;
    return SLAM_OK;
}

int slam_kf_sc_read(slam_kf_t *s, int id, uint8_t *desc, int cap, int *n_rings, int *n_sectors)
{
    SLAM_REQUIRE(s && kf_live(s, id) && cap >= 0 && (desc || cap == 0), SLAM_E_INVALID, "slam_kf_sc_read: bad arguments");
    const Keyframe &kf = s->kfs[id];
    SLAM_REQUIRE(kf.sc.p, SLAM_E_INVALID, "slam_kf_sc_read: keyframe %d has no descriptor yet", id);
    const int nc = s->sp.n_rings * s->sp.n_sectors;
    SLAM_REQUIRE(cap == 0 || cap >= nc, SLAM_E_INVALID, "slam_kf_sc_read: room for %d bytes, the descriptor has %d", cap, nc);
    if (cap) SLAM_HIP(hipMemcpy(desc, kf.sc.p, (size_t)nc, hipMemcpyDeviceToHost));
    if (n_rings) *n_rings = s->sp.n_rings;
    if (n_sectors) *n_sectors = s->sp.n_sectors;
    return SLAM_OK;
}

int slam_kf_sc_match(slam_kf_t *s, const int *queries, int nq, slam_kf_sc_match_t *out, slam_stream_t stream)
{
    SLAM_REQUIRE(s && nq >= 0 && (nq == 0 || (queries && out)), SLAM_E_INVALID, "slam_kf_sc_match: bad arguments");
    const int count = (int)s->kfs.size();
    for (int q = 0; q < nq; ++q)
        SLAM_REQUIRE(kf_live(s, queries[q]), SLAM_E_INVALID, "slam_kf_sc_match: query %d names keyframe %d, the store holds %d (removed ones are refused)",
                     q, queries[q], count);
    if (nq == 0) return SLAM_OK;
    const size_t pairs = (size_t)nq * count;
    SLAM_REQUIRE(pairs <= (size_t)INT_MAX, SLAM_E_INVALID, "slam_kf_sc_match: %d queries against %d keyframes are more pairs than one launch takes", nq,
                 count);
    SLAM_TRY(slam_kf_sc_compute(s, -1, stream)); // the missing descriptors; waits
    // s->work and its pinned mirror: descriptor pointers | queries | results, each from a multiple of 256 bytes
    const size_t ptr_b = sizeof(uint8_t *) * (size_t)count, q_off = (ptr_b + 255) & ~(size_t)255;
    const size_t out_off = q_off + ((sizeof(int) * (size_t)nq + 255) & ~(size_t)255), out_b = sizeof(slam_kf_sc_match_t) * pairs;
    SLAM_TRY(reserve_quarter(s->work, out_off + out_b));
    char *host = static_cast<char *>(pinned_scratch(out_off + out_b));
    SLAM_REQUIRE(host, SLAM_E_NOMEM, "slam_kf_sc_match: no pinned staging memory");
    char           *dev = static_cast<char *>(s->work.p);
    const uint8_t **ptrs = reinterpret_cast<const uint8_t **>(host);
    for (int k = 0; k < count; ++k) ptrs[k] = s->kfs[k].removed ? nullptr : s->kfs[k].sc.as<const uint8_t>();
    std::memcpy(host + q_off, queries, sizeof(int) * (size_t)nq);
    hipStream_t st = as_stream(stream);
    SLAM_HIP(hipMemcpyAsync(dev, host, out_off, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kf_sc_match_kernel, dim3((unsigned)pairs), dim3(kScThreads), 0, st, reinterpret_cast<const uint8_t *const *>(dev),
                       reinterpret_cast<const int *>(dev + q_off), reinterpret_cast<slam_kf_sc_match_t *>(dev + out_off), count, s->sp.n_rings,
                       s->sp.n_sectors);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(host + out_off, dev + out_off, out_b, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    std::memcpy(out, host + out_off, out_b);
    return SLAM_OK;
}

} // extern "C"
