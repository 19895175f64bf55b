// What abi.cc, abi_gptq.cc and abi_chain.cc share and nothing else sees: the workspace handle, the view of a GPTQ handle and the
// pointer casts of the C-ABI wrappers.
#pragma once
#include "common.h"

struct FerrumHipWorkspace {
    float* ptr = nullptr;
    size_t bytes = 0;
};

struct FerrumHipGptq;
namespace fh {
struct W4Device;
const W4Device* gptq_device(const FerrumHipGptq* h);      // abi_gptq.cc: the projection behind a handle
bool gptq_is_shape_only(const FerrumHipGptq* h);          // made by ferrum_hip_gptq_shape_only: dims, no weights
}

#define H(p) reinterpret_cast<__half*>(p)
#define CH(p) reinterpret_cast<const __half*>(p)
#define ST(s) reinterpret_cast<hipStream_t>(s)
