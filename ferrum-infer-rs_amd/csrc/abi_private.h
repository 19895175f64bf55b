// What abi.cc and abi_gptq.cc share and nothing else sees: the workspace handle and the pointer casts of the C-ABI wrappers.
#pragma once
#include "common.h"

struct FerrumHipWorkspace {
    float* ptr = nullptr;
    size_t bytes = 0;
};

#define H(p) reinterpret_cast<__half*>(p)
#define CH(p) reinterpret_cast<const __half*>(p)
#define ST(s) reinterpret_cast<hipStream_t>(s)
