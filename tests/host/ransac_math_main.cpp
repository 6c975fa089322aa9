// Stand-alone driver of sfd2_amd/csrc/ransac_math.h, the HIP-free part of what the RANSAC kernels share (tests/test_ransac_math_host.py
// builds it with -fsanitize=address,undefined, feeds it one request per line and compares the answers with numpy and the restatements):
//   chol N lambda s[0 .. N(N+1)/2 + N)      -> "ok d[0 .. N)" or "fail"      chol_solve<N> on a heap array of exactly that length
//   sample K seed trial n                   -> the K indices                  sample_k<K>
//   enough K trials min max conf n best_cnt -> 0 / 1                          ransac_enough with ratio^K spelt out as in the kernels
// Numbers are read with strtod / strtoull, so hexadecimal floats, nan and inf pass through unchanged.
#include "../../sfd2_amd/csrc/ransac_math.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

struct Conf {
    int64_t min_trials, max_trials;
    double confidence;
};

static double next_double(std::istringstream &in)
{
    std::string w;
    in >> w;
    return std::strtod(w.c_str(), nullptr);
}
static long long next_int(std::istringstream &in)
{
    std::string w;
    in >> w;
    return std::strtoll(w.c_str(), nullptr, 0);
}

template <int N> void chol(std::istringstream &in)
{
    constexpr int NS = normal_size<N>();
    const double lambda = next_double(in);
    // on the heap at exactly its length: a read past the gradient is an AddressSanitizer report
    std::unique_ptr<double[]> heap(new double[NS]);
    for (int i = 0; i < NS; ++i) heap[i] = next_double(in);
    double d[N];
    if (!chol_solve<N>(*reinterpret_cast<const double(*)[NS]>(heap.get()), lambda, d)) {
        std::printf("fail\n");
        return;
    }
    std::printf("ok");
    for (int i = 0; i < N; ++i) std::printf(" %a", d[i]);
    std::printf("\n");
}

template <int K> void sample(std::istringstream &in)
{
    std::string w;
    in >> w;
    const uint64_t seed = std::strtoull(w.c_str(), nullptr, 0);
    const int64_t trial = next_int(in);
    const int n = (int)next_int(in);
    int id[K];
    sample_k<K>(seed, trial, n, id);
    for (int i = 0; i < K; ++i) std::printf(i ? " %d" : "%d", id[i]);
    std::printf("\n");
}

static void enough(std::istringstream &in, int K)
{
    const int64_t trials = next_int(in);
    Conf conf;
    conf.min_trials = next_int(in);
    conf.max_trials = next_int(in);
    conf.confidence = next_double(in);
    const int n = (int)next_int(in), best_cnt = (int)next_int(in);
    bool stop = false;
    if (K == 3) stop = ransac_enough(trials, conf, n, best_cnt, [](double r) { return r * r * r; });
    else if (K == 4) stop = ransac_enough(trials, conf, n, best_cnt, [](double r) { const double r2 = r * r; return r2 * r2; });
    else if (K == 5) stop = ransac_enough(trials, conf, n, best_cnt, [](double r) { return r * r * r * r * r; });
    else stop = ransac_enough(trials, conf, n, best_cnt, [](double r) { const double r2 = r * r, r4 = r2 * r2; return r4 * r2 * r; });
    std::printf("%d\n", stop ? 1 : 0);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        const int k = cmd.empty() ? 0 : (int)next_int(in);
        if (cmd == "chol" && k == 5) chol<5>(in);
        else if (cmd == "chol" && k == 6) chol<6>(in);
        else if (cmd == "chol" && k == 7) chol<7>(in);
        else if (cmd == "chol" && k == 8) chol<8>(in);
        else if (cmd == "sample" && k == 3) sample<3>(in);
        else if (cmd == "sample" && k == 5) sample<5>(in);
        else if (cmd == "enough") enough(in, k);
        else { std::fprintf(stderr, "bad request: %s\n", line.c_str()); return 2; }
    }
    std::printf("ransac_math: done\n");
    return 0;
}
