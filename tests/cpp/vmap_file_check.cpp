// vmap_file_check.cpp -- the snapshot file's parser alone (slam_amd/csrc/vmap_file.hpp, docs/VOXEL_MAP.md section 10.4), as a
// program of its own so that the host sanitizers see it: tests/test_vmap_snapshot.py builds it with
// -fsanitize=address,undefined and runs it over good, malformed and truncated files.  Of the project it includes the one
// header; it is never loaded into Python and never runs on a GPU.
//   vmap_file_check DIR     one line per regular file of DIR in name order: "<name> ok <n> <n_points> <flags>" or
//                           "<name> invalid"; exit status 0 unless DIR cannot be read.  A file that parses is also walked
//                           record by record and written again: the rebuilt bytes must equal the file's ("... ok" becomes
//                           "... differs" otherwise).
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>

#include "vmap_file.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    DIR *d = opendir(argv[1]);
    if (!d) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<std::string> names;
    while (dirent *e = readdir(d)) names.push_back(e->d_name);
    closedir(d);
    std::sort(names.begin(), names.end());
    for (const std::string &name : names) {
        const std::string path = std::string(argv[1]) + "/" + name;
        struct stat       st;
        if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) continue;
        std::vector<uint8_t> bytes;
        std::string          why;
        if (vmap_file::read_all(path.c_str(), &bytes, &why) != 0) {
            std::printf("%s unreadable\n", name.c_str());
            continue;
        }
        vmap_file::View v;
        if (!vmap_file::parse(bytes.data(), bytes.size(), &v, &why)) {
            std::printf("%s invalid\n", name.c_str());
            continue;
        }
        // every array through typed copies, as the loader hands them on, and back through the writer
        const size_t          N = (size_t)v.meta.n;
        std::vector<uint64_t> key(N);
        std::vector<uint32_t> count(N), seen(v.seen ? N : 0), miss(v.miss ? N : 0);
        std::vector<int64_t>  sums(3 * N), E(v.E ? 3 * N : 0), M(v.M ? 6 * N : 0);
        if (N) {
            std::memcpy(key.data(), v.key, N * 8), std::memcpy(count.data(), v.count, N * 4), std::memcpy(sums.data(), v.sums, N * 24);
            if (v.seen) std::memcpy(seen.data(), v.seen, N * 4), std::memcpy(miss.data(), v.miss, N * 4);
            if (v.E) std::memcpy(E.data(), v.E, N * 24), std::memcpy(M.data(), v.M, N * 48);
        }
        const std::vector<uint8_t> again = vmap_file::build(v.meta, key.data(), count.data(), sums.data(), seen.data(), miss.data(), E.data(), M.data());
        std::printf("%s %s %lld %lld %u\n", name.c_str(), again == bytes ? "ok" : "differs", (long long)v.meta.n, (long long)v.meta.n_points,
                    v.meta.flags);
    }
    return 0;
}
