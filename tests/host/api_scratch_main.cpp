// Stand-alone check of sfd2_amd/csrc/api_scratch.h (tests/test_api_scratch_host.py builds it with -fsanitize=address,undefined and runs it).
// Every array lives on the heap at exactly its logical length, so a read past its end is an AddressSanitizer report.
// After its own checks it answers one request per line of standard input (numbers through strtod / strtoll: hexadecimal floats pass unchanged):
//   limits p_all_inliers confidence min_num_trials max_num_trials cap -> "min_trials max_trials"        trial_limits
//   check confidence min_inlier_ratio min_num_trials max_num_trials   -> ransac_conf_error's text, or "ok"
#include "../../sfd2_amd/csrc/api_scratch.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <iostream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

template <typename T> std::unique_ptr<T[]> heap(std::initializer_list<T> v)
{
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

template <typename T> void finite_cases()
{
    const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
    CHECK(all_finite(static_cast<const T *>(nullptr), 0));
    CHECK(all_finite(heap<T>({T(0), T(-1.5), std::numeric_limits<T>::max()}).get(), 3));
    CHECK(!all_finite(heap<T>({T(0), nan}).get(), 2));
    CHECK(!all_finite(heap<T>({inf, T(0)}).get(), 2));
    CHECK(!all_finite(heap<T>({T(0), T(1), -inf}).get(), 3));
    CHECK(all_finite(heap<T>({T(0), nan}).get(), 1));          // the count bounds what is looked at
}

static double next_double(std::istringstream &in)
{
    std::string w;
    in >> w;
    return std::strtod(w.c_str(), nullptr);
}
static int64_t next_int(std::istringstream &in)
{
    std::string w;
    in >> w;
    return std::strtoll(w.c_str(), nullptr, 0);
}

int main()
{
    // ---- align256, Carve
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
    {
        Carve c;
        const size_t sizes[] = {0, 1, 256, 257}, advance[] = {256, 256, 256, 512};
        size_t sum = 0;
        for (int i = 0; i < 4; ++i) {
            const size_t o = c.take(sizes[i]);
            CHECK(o == sum && o % 256 == 0);                    // take returns the offset BEFORE advancing
            sum += advance[i];
            CHECK(c.off == sum);
        }
        Carve seeded{512};
        CHECK(seeded.take(8) == 512 && seeded.off == 768);
    }
    // ---- at
    {
        std::unique_ptr<char[]> block(new char[512]);
        CHECK(reinterpret_cast<char *>(at<int64_t>(block.get(), 256)) == block.get() + 256);
        CHECK(reinterpret_cast<const char *>(at<const float>(block.get(), 0)) == block.get());
    }
    // ---- monotone: n + 1 offsets
    CHECK(monotone(heap<int64_t>({0}).get(), 0));
    CHECK(!monotone(heap<int64_t>({1}).get(), 0));
    CHECK(monotone(heap<int64_t>({0, 0, 3}).get(), 2));
    CHECK(!monotone(heap<int64_t>({0, 2, 1}).get(), 2));
    CHECK(monotone(heap<int64_t>({0, 5}).get(), 1));
    CHECK(!monotone(heap<int64_t>({-1, 5}).get(), 1));
    // ---- in_range / first_outside
    {
        const int hi = 7;
        CHECK(in_range(nullptr, 0, hi) && first_outside(nullptr, 0, hi) == 0);
        CHECK(!in_range(heap<int32_t>({-1}).get(), 1, hi));
        CHECK(in_range(heap<int32_t>({hi - 1}).get(), 1, hi));
        CHECK(!in_range(heap<int32_t>({hi}).get(), 1, hi));
        CHECK(in_range(heap<int32_t>({0, 3, hi - 1}).get(), 3, hi));
        CHECK(first_outside(heap<int32_t>({0, 3, hi - 1}).get(), 3, hi) == 3);
        CHECK(first_outside(heap<int32_t>({0, hi, -1}).get(), 3, hi) == 1);      // the first one
        CHECK(first_outside(heap<int32_t>({0, 1, -1}).get(), 3, hi) == 2);
        CHECK(!in_range(heap<int32_t>({0}).get(), 1, 0));                        // an empty range holds nothing
    }
    // ---- all_finite, float and double
    finite_cases<float>();
    finite_cases<double>();
    // ---- the trial limits: the parts that need no reference (the grid against the restatement comes in through the requests)
    CHECK(floored_ratio(0.5000099) == 0.5 && floored_ratio(0.25) == 0.25 && floored_ratio(1.0) == 1.0 && floored_ratio(0.0) == 0.0);
    CHECK(num_trials(0.5, 1.0) == 1e300 && num_trials(0.0, 0.999) == 1e300 && num_trials(1.0, 0.999) == 1.0);
    CHECK(ransac_conf_error(0.999, 0.25, 0, 10000) == nullptr && ransac_conf_error(0.0, 1.0, 0, 1) == nullptr);
    CHECK(ransac_conf_error(std::numeric_limits<double>::quiet_NaN(), 0.25, 0, 10000) != nullptr);
    if (failures) return 1;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "limits") {
            const double p_all = next_double(in), confidence = next_double(in);
            const int64_t mn = next_int(in), mx = next_int(in), cap = next_int(in);
            const TrialLimits t = trial_limits(confidence, mn, mx, cap, p_all);
            std::printf("%lld %lld\n", (long long)t.min_trials, (long long)t.max_trials);
        } else if (cmd == "check") {
            const double confidence = next_double(in), ratio = next_double(in);
            const int64_t mn = next_int(in), mx = next_int(in);
            const char *bad = ransac_conf_error(confidence, ratio, mn, mx);
            std::printf("%s\n", bad ? bad : "ok");
        } else {
            std::fprintf(stderr, "bad request: %s\n", line.c_str());
            return 2;
        }
    }
    std::puts("api_scratch: ok");
    return 0;
}
