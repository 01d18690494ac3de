// What the stand-alone sanitizer programs (abi_args*.cpp) share: the failure count and the expectation of one call's status.
#pragma once
#include <cstdio>

static int failures = 0;
#define EXPECT(call, want)                                                                  \
    do {                                                                                    \
        const long long got_ = (long long)(call);                                          \
        if (got_ != (long long)(want)) {                                                    \
            std::printf("FAIL %s:%d  %s = %lld, expected %s\n", __FILE__, __LINE__, #call, got_, #want); \
            ++failures;                                                                     \
        }                                                                                   \
    } while (0)
