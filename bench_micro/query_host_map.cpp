// query_host_map.cpp -- the host-side comparator of bench_micro/query_timing.py: the k-mer lookup a caller of the library had to write
// before cdbg_query, with the structure bcalm_tools keeps its end k-mers in (std::unordered_map<std::string, ...>), single thread.
//   query_host_map <unitigs, one per line> <queries, one per line> <k>   ->   one JSON line
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

static std::string rc(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: query_host_map unitigs.txt queries.txt k\n"); return 2; }
    const size_t k = (size_t)atoi(argv[3]);
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    std::vector<std::string> ut, qs; std::string line; size_t npos = 0;
    { std::ifstream f(argv[1]); while (std::getline(f, line)) { if (line.size() >= k) npos += line.size() - k + 1; ut.push_back(line); } }
    { std::ifstream f(argv[2]); while (std::getline(f, line)) qs.push_back(line); }
    const auto t0 = clk::now();
    std::unordered_map<std::string, std::pair<uint32_t, uint32_t>> idx;
    idx.reserve(npos);
    for (size_t u = 0; u < ut.size(); ++u)
        for (size_t o = 0; o + k <= ut[u].size(); ++o) {
            std::string x = ut[u].substr(o, k), r = rc(x);
            idx.emplace(r < x ? r : x, std::make_pair((uint32_t)u, (uint32_t)o));
        }
    const auto t1 = clk::now();
    uint64_t n = 0, found = 0;
    for (const std::string& q : qs)
        for (size_t p = 0; p + k <= q.size(); ++p) {
            std::string x = q.substr(p, k), r = rc(x);
            found += idx.count(r < x ? r : x); ++n;
        }
    const auto t2 = clk::now();
    printf("{\"map_kmers\": %zu, \"build_s\": %.3f, \"lookups\": %llu, \"found\": %llu, \"lookup_s\": %.3f, \"mkmers_s\": %.3f}\n", idx.size(), secs(t0, t1),
           (unsigned long long)n, (unsigned long long)found, secs(t1, t2), n / secs(t1, t2) / 1e6);
    return 0;
}
