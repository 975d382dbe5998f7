// Hybrid fusion (hybrid_fuse.hip): the set union of two candidate lists per query, and the ranking of a ragged candidate list by the
// fused score f32(f32(w_d * dense) + f32(w_s * sparse)) with the certificate of the exact hybrid search.
#pragma once
#include "common.h"

struct HybridStatus {                   // device words of a call: what the kernels found wrong (~0: nothing)
    unsigned long long first_bad_b;     // smallest flat position of list B whose sparse position maps to no dense document
    unsigned long long first_bad_a;     // smallest flat position of list A (or of the ranked list) that is outside the index
};

#define HF_THREADS 256
#define HF_EMPTY 0xffffffffu            // an unused slot of a sorted list: sorts behind every dense position
