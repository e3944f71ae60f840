// shufflecheck.cpp -- shuffle_index of so100_learn.hpp (what the kernel so100_learn_shuffle calls per position) on the host, behind a C
// interface for ctypes (part of liblearncheck.so: tests/hostlibs.py; called by tests/update_support.py).  Test scaffolding only.
#include "../../so100_mujoco_rl_amd/csrc/so100_task.hpp"       // philox4x32: before so100_learn.hpp, which has the shuffle only behind it
#include "../../so100_mujoco_rl_amd/csrc/so100_learn.hpp"

extern "C" {

// out[i] = the row at position i, for every i in [0, n)
void sc_shuffle(unsigned long long seed, unsigned epoch, long n, long* out) {
    for (long i = 0; i < n; i++) out[i] = (long)so100::learn::shuffle_index((uint32_t)i, (uint32_t)n, seed, epoch);
}

// `epochs` permutations of [0, n) from epoch0 on, as one [epochs][n] int32 table (the uniformity tests draw thousands)
void sc_shuffle_epochs(unsigned long long seed, unsigned epoch0, int epochs, int n, int* out) {
    for (int e = 0; e < epochs; e++)
        for (int i = 0; i < n; i++) out[(long)e*n + i] = (int)so100::learn::shuffle_index((uint32_t)i, (uint32_t)n, seed, epoch0 + (unsigned)e);
}

}  // extern "C"
