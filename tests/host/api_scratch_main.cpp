// Stand-alone check of sfd2_amd/csrc/api_scratch.h (tests/test_api_scratch_host.py builds it with -fsanitize=address,undefined and runs it).
// Every array lives on the heap at exactly its logical length, so a read past its end is an AddressSanitizer report.
#include "../../sfd2_amd/csrc/api_scratch.h"

#include <cstdio>
#include <initializer_list>
#include <limits>
#include <memory>

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
    if (failures) return 1;
    std::puts("api_scratch: ok");
    return 0;
}
