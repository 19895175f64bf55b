// The one way a W4Device is filled and freed: the dims of the packed "w4t" layout (w4_repack.cc), the device upload of a
// repacked projection, and the expert stack that is reserved once and filled expert by expert.  Used by the runner's weight
// setters (runner_model.hip) and by the op-level GPTQ handles (abi_gptq.cc).
#pragma once
#include "kernels.h"

namespace fh {

// packed sizes of ONE projection / expert: dwords of qw, halves of sc (and of zp)
inline size_t w4_qw_words(int n64, int G) { return (size_t)n64 * G * 4 * 64 * 4; }
inline size_t w4_sc_elems(int n64, int G) { return (size_t)n64 * G * 16 * 4; }

inline void w4_set_dims(W4Device* w, int k, int n, int num_experts, bool fused_gate_up) {
    w->k = k; w->n = n; w->n64 = (n + 63) / 64; w->G = k / 128; w->num_experts = num_experts; w->fused_gate_up = fused_gate_up;
}

// fused gate_up column order: supertile st = [gate 32st.. | up I+32st..]  (w4_repack.cc)
std::vector<int32_t> gate_up_col_perm(int n);

void w4_free(W4Device& w);                                              // every device buffer; w is left empty
int w4_upload(const W4HostPacked& hp, W4Device* w);                    // a single projection (whatever w held is freed first)
int w4_upload_perm(const std::vector<int32_t>& perm, W4Device* w);     // act-order input permutation and its inverse
// Expert stack: one allocation for E experts (a no-op when the stack exists), then one expert at a time.  The stack gets a
// zero-point array as soon as one expert needs it; symmetric experts of such a stack carry the explicit zero point 8.0.
int w4_stack_reserve(W4Device* w, int k, int n, int E, bool fused);
int w4_stack_put(W4Device* w, int expert, const W4HostPacked& hp);

}  // namespace fh
