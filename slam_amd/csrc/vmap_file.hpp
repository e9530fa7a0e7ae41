// vmap_file.hpp -- the voxel map's snapshot file, version 1 (docs/VOXEL_MAP.md section 10.4): parser and writer in plain
// host C++.  No HIP, no device types, nothing of the library: voxmap.hip includes it, and tests/cpp/vmap_file_check.cpp
// compiles it alone under the host sanitizers.  Little-endian throughout; a host of the other order is refused at compile time.
//
//   header, 96 bytes   0 magic "SLAMVMAP"   8 u32 version = 1   12 u32 flags (bit 0 carve planes, bit 1 moments)   16 f64 leaf
//                      24 i64 n   32 i64 n_points   40 i32 min_points   44 i32 max_miss_num   48 i32 max_miss_den   52 u32 zero
//                      56 f64 flat_ratio   64 f64 line_ratio   72 f64 epsilon   80 u64 payload bytes   88 u64 zero
//                      (40 .. 79 all zero without bit 1)
//   payload            key u64[n]; count u32[n], zero-padded to 8 bytes; sums i64[3 n]; with bit 0 seen u32[n], miss u32[n];
//                      with bit 1 E i64[3 n], M i64[6 n]
// There is no checksum: a flipped bit inside a sum is not noticed.  What is checked is the structure (parse() below).
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "vmap_file.hpp reads and writes little-endian files with memcpy: a little-endian host is assumed"
#endif

namespace vmap_file {

constexpr size_t   kHeaderBytes = 96;
constexpr uint32_t kVersion = 1, kCarve = 1u, kMoments = 2u;
constexpr int64_t  kMaxVoxels = 1ll << 30;
constexpr uint64_t kFieldMask = (1ull << 21) - 1;

struct Meta {
    uint32_t flags = 0;
    double   leaf = 0.0;
    int64_t  n = 0, n_points = 0;
    int32_t  min_points = 0, max_miss_num = 0, max_miss_den = 0;
    double   flat_ratio = 0.0, line_ratio = 0.0, epsilon = 0.0;
};
// a parsed file: the header's fields and where each array starts inside the buffer (null where the file has none).  The
// buffer is 8-byte aligned when it comes from operator new, and every section's offset is a multiple of its element's size.
struct View {
    Meta           meta;
    const uint8_t *key = nullptr, *count = nullptr, *sums = nullptr, *seen = nullptr, *miss = nullptr, *E = nullptr, *M = nullptr;
};

template <class T>
inline T get(const uint8_t *p)
{
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
}
template <class T>
inline void put(uint8_t *p, T v)
{
    std::memcpy(p, &v, sizeof(T));
}

inline uint64_t count_bytes(int64_t n) { return ((uint64_t)n * 4 + 7) & ~7ull; }
inline uint64_t payload_bytes(int64_t n, uint32_t flags)
{
    return (uint64_t)n * 8 + count_bytes(n) + (uint64_t)n * 24 + ((flags & kCarve) ? (uint64_t)n * 8 : 0) + ((flags & kMoments) ? (uint64_t)n * 72 : 0);
}

// section 1's keys: not all ones, bit 63 clear, no 21-bit field above 2^21 - 2
inline bool key_valid(uint64_t k)
{
    if (k >> 63) return false;
    for (int s = 0; s < 63; s += 21)
        if (((k >> s) & kFieldMask) > kFieldMask - 1) return false;
    return true;
}

// the parameters slam_vmap_enable_distributions accepts (a NaN fails every comparison)
inline bool dist_params_valid(const Meta &m)
{
    return m.min_points >= 1 && m.flat_ratio >= 0 && m.line_ratio >= 0 && m.epsilon > 0 && m.max_miss_num >= 0 && m.max_miss_den >= 0;
}

// Whether buf[0 .. len) is a valid file; `why` (nullable) names the first rule that failed.  Nothing beyond len is read.
inline bool parse(const uint8_t *buf, size_t len, View *out, std::string *why = nullptr)
{
    auto fail = [&](const char *w) {
        if (why) *why = w;
        return false;
    };
    if (!buf || len < kHeaderBytes) return fail("shorter than the header");
    if (std::memcmp(buf, "SLAMVMAP", 8) != 0) return fail("the magic is not SLAMVMAP");
    if (get<uint32_t>(buf + 8) != kVersion) return fail("the version is not 1");
    Meta m;
    m.flags = get<uint32_t>(buf + 12);
    if (m.flags & ~(kCarve | kMoments)) return fail("unknown flags");
    m.leaf = get<double>(buf + 16);
    m.n = get<int64_t>(buf + 24);
    m.n_points = get<int64_t>(buf + 32);
    m.min_points = get<int32_t>(buf + 40), m.max_miss_num = get<int32_t>(buf + 44), m.max_miss_den = get<int32_t>(buf + 48);
    m.flat_ratio = get<double>(buf + 56), m.line_ratio = get<double>(buf + 64), m.epsilon = get<double>(buf + 72);
    if (get<uint32_t>(buf + 52) != 0 || get<uint64_t>(buf + 88) != 0) return fail("a reserved field is not zero");
    if (!(std::isfinite(m.leaf) && m.leaf > 0)) return fail("the leaf is not positive and finite");
    if (m.flags & kMoments) {
        if (!(m.leaf <= 8.0)) return fail("a leaf above 8 m with moments");
        if (!dist_params_valid(m)) return fail("distribution parameters that enable_distributions refuses");
    } else {
        for (size_t o = 40; o < 80; ++o)
            if (buf[o]) return fail("distribution parameters without the moments flag");
    }
    if (m.n < 0 || m.n > kMaxVoxels) return fail("n outside 0 .. 2^30");
    const uint64_t payload = payload_bytes(m.n, m.flags);
    if (get<uint64_t>(buf + 80) != payload) return fail("the header's payload figure does not follow from n and the flags");
    if ((uint64_t)len != kHeaderBytes + payload) return fail("the length is not 96 + payload");
    const size_t N = (size_t)m.n;
    View         v;
    v.meta = m;
    const uint8_t *p = buf + kHeaderBytes;
    v.key = p, p += N * 8;
    v.count = p, p += count_bytes(m.n);
    v.sums = p, p += N * 24;
    if (m.flags & kCarve) v.seen = p, p += N * 4, v.miss = p, p += N * 4;
    if (m.flags & kMoments) v.E = p, p += N * 24, v.M = p, p += N * 48;
    uint64_t prev = 0, total = 0;
    for (size_t i = 0; i < N; ++i) {
        const uint64_t k = get<uint64_t>(v.key + 8 * i);
        if (!key_valid(k)) return fail("a key that section 1 does not allow");
        if (i && k <= prev) return fail("keys not strictly ascending");
        prev = k;
        const uint32_t c = get<uint32_t>(v.count + 4 * i);
        if (c == 0) return fail("a count of zero");
        total += c; // n <= 2^30 counts below 2^32: no wrap
    }
    for (size_t o = N * 4; o < count_bytes(m.n); ++o)
        if (v.count[o]) return fail("the padding is not zero");
    if (m.n_points < 0 || total != (uint64_t)m.n_points) return fail("n_points is not the sum of the counts");
    if (out) *out = v;
    return true;
}

// The file's bytes from the arrays the key-ordered readers return (seen / miss and E / M by the flags; null otherwise).
inline std::vector<uint8_t> build(const Meta &m, const uint64_t *key, const uint32_t *count, const int64_t *sums, const uint32_t *seen,
                                  const uint32_t *miss, const int64_t *E, const int64_t *M)
{
    const size_t         N = (size_t)m.n;
    const uint64_t       payload = payload_bytes(m.n, m.flags);
    std::vector<uint8_t> b(kHeaderBytes + (size_t)payload, 0);
    std::memcpy(b.data(), "SLAMVMAP", 8);
    put<uint32_t>(&b[8], kVersion), put<uint32_t>(&b[12], m.flags);
    put<double>(&b[16], m.leaf), put<int64_t>(&b[24], m.n), put<int64_t>(&b[32], m.n_points);
    if (m.flags & kMoments) {
        put<int32_t>(&b[40], m.min_points), put<int32_t>(&b[44], m.max_miss_num), put<int32_t>(&b[48], m.max_miss_den);
        put<double>(&b[56], m.flat_ratio), put<double>(&b[64], m.line_ratio), put<double>(&b[72], m.epsilon);
    }
    put<uint64_t>(&b[80], payload);
    uint8_t *p = b.data() + kHeaderBytes;
    auto     add = [&](const void *src, size_t bytes, size_t room) {
        if (bytes) std::memcpy(p, src, bytes);
        p += room;
    };
    add(key, N * 8, N * 8);
    add(count, N * 4, (size_t)count_bytes(m.n));
    add(sums, N * 24, N * 24);
    if (m.flags & kCarve) add(seen, N * 4, N * 4), add(miss, N * 4, N * 4);
    if (m.flags & kMoments) add(E, N * 24, N * 24), add(M, N * 48, N * 48);
    return b;
}

// 0, or errno with *why set (nullable)
inline int read_all(const char *path, std::vector<uint8_t> *out, std::string *why = nullptr)
{
    auto fail = [&](const char *what) {
        const int e = errno ? errno : EIO;
        if (why) *why = std::string(what) + " " + (path ? path : "(null)") + ": " + std::strerror(e);
        return e;
    };
    errno = 0;
    std::FILE *f = path ? std::fopen(path, "rb") : nullptr;
    if (!f) {
        if (!path) errno = EINVAL;
        return fail("cannot open");
    }
    out->clear();
    uint8_t chunk[1 << 16];
    size_t  got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) out->insert(out->end(), chunk, chunk + got);
    if (std::ferror(f)) {
        const int e = fail("cannot read");
        std::fclose(f);
        return e;
    }
    std::fclose(f);
    return 0;
}

inline int write_all(const char *path, const std::vector<uint8_t> &b, std::string *why = nullptr)
{
    auto fail = [&](const char *what) {
        const int e = errno ? errno : EIO;
        if (why) *why = std::string(what) + " " + (path ? path : "(null)") + ": " + std::strerror(e);
        return e;
    };
    errno = 0;
    std::FILE *f = path ? std::fopen(path, "wb") : nullptr;
    if (!f) {
        if (!path) errno = EINVAL;
        return fail("cannot open");
    }
    if (!b.empty() && std::fwrite(b.data(), 1, b.size(), f) != b.size()) {
        const int e = fail("cannot write");
        std::fclose(f);
        return e;
    }
    if (std::fclose(f) != 0) return fail("cannot close");
    return 0;
}

} // namespace vmap_file
