// sjd_switches.h -- the environment switches of the EXPERIMENTAL library (libsjd_hip_exp.so), each selecting an alternative form that a test
// compares the product's against.  Read once per process, here and nowhere else: the product library is compiled without this header's
// contents and never looks at the environment.
#pragma once
#ifdef SJD_EXPERIMENTAL
#include <stdlib.h>

struct sjd_switches {
    bool k1_no_direct;      // SJD_K1_NO_DIRECT set: one key split still runs k1_partial + k1_combine (16-bit and fp8 caches)
    bool k1_ring;           // SJD_K1_RING=0 clears it: the shared-tile shapes run on k1_partial_shared instead of the ring kernel

    static const sjd_switches &get()
    {
        static const sjd_switches s = [] {
            const char *ring = getenv("SJD_K1_RING");
            return sjd_switches{getenv("SJD_K1_NO_DIRECT") != nullptr, !(ring && ring[0] == '0')};
        }();
        return s;
    }
};
#endif  // SJD_EXPERIMENTAL
