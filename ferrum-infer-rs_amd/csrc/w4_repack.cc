// Load-time repack of GPTQ-INT4 weights into the "w4t" tile layout the gfx950 INT4 GEMMs stream (host only; design: w4_gemm.h).
#include <algorithm>
#include <vector>

#include "common.h"
#include "w4_upload.h"

namespace fh {

// ───────────────────────────── repacked layout ─────────────────────────────
// qw : u32  [n64][G][4 nt][64 lanes][4 dwords]          (G = K/128, n64 = ceil(N/64))
//      lane l=(a=l>>4, b=l&15), column n = st·64 + nt·16 + b.  Dwords come in pairs: (d0,d1) carry
//      k-steps 0 ("lo") and 1 ("hi") of the group, (d2,d3) k-steps 2 and 3.  Element j (0..7) of k-step s
//      is k = g·128 + 32s + 8a + j.  Inside dword d_{2p+h} (h = j>>2, jj = j&3) the LO k-step sits in
//      nibbles {0,4,2,6}[jj] and the HI k-step in nibbles {1,5,3,7}[jj]: a lo nibble masked in place is
//      the fp16 1024+q, a hi nibble masked in place is 1024+16q — 5 VALU ops expand a dword (see below).
// sc : f16  [n64][G][16 b][4 nt]                         group scale of column st·64+nt·16+b
// zp : f16  [n64][G][16 b][4 nt]  (only when asymmetric)  value (z+1) as fp16

// nibble slot of (hi k-step?, jj) inside a dword
static inline int nibble_slot(int hi, int jj) {
    static const int lo_slots[4] = {0, 4, 2, 6}, hi_slots[4] = {1, 5, 3, 7};
    return hi ? hi_slots[jj] : lo_slots[jj];
}

static inline uint16_t f32_to_f16_bits(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

// fused gate_up column order: supertile st = [gate 32st.. | up I+32st..]
std::vector<int32_t> gate_up_col_perm(int n) {
    std::vector<int32_t> p(n);
    const int I = n / 2;
    for (int st = 0; st < n / 64; st++)
        for (int c = 0; c < 64; c++) p[st * 64 + c] = c < 32 ? st * 32 + c : I + st * 32 + (c - 32);
    return p;
}

int w4_repack_host(const int32_t* qweight, const float* scales, const int32_t* qzeros,
                   const int32_t* g_idx, const int32_t* col_perm, int group_size, int k, int n,
                   W4HostPacked* out) {
    FH_REQUIRE(k % 128 == 0, "w4 repack: K=%d must be a multiple of 128", k);
    FH_REQUIRE(n % 8 == 0, "w4 repack: N=%d must be a multiple of 8", n);
    FH_REQUIRE(group_size > 0 && group_size % 128 == 0 && k % group_size == 0,
               "w4 repack: group_size=%d must be a multiple of 128 dividing K=%d", group_size, k);
    const int G = k / 128, n64 = (n + 63) / 64;
    const int num_groups = k / group_size;

    // act-order: rows sorted by g_idx so that quant groups become contiguous
    // (same transform the reference applies before Marlin: cuda/quant.rs:434 + gather_columns).
    std::vector<int32_t> perm;
    bool use_perm = false;
    if (g_idx) {
        bool sequential = true;
        for (int i = 0; i < k; i++)
            if (g_idx[i] != i / group_size) { sequential = false; break; }
        if (!sequential) {
            use_perm = true;
            perm.resize(k);
            for (int i = 0; i < k; i++) perm[i] = i;
            std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return g_idx[x] < g_idx[y]; });
            std::vector<int> counts(num_groups, 0);
            for (int i = 0; i < k; i++) {
                FH_REQUIRE(g_idx[i] >= 0 && g_idx[i] < num_groups, "w4 repack: g_idx[%d]=%d out of range", i, g_idx[i]);
                counts[g_idx[i]]++;
            }
            for (int g = 0; g < num_groups; g++)
                FH_REQUIRE(counts[g] == group_size, "w4 repack: act-order groups must be balanced (group %d has %d rows)", g, counts[g]);
        }
    }
    // symmetric ⇔ every zero nibble is 7 (zero point 8), the `sym=true` canonical form
    // (ferrum-quantization/src/native_safetensors.rs:1242).
    bool symmetric = true;
    for (long i = 0; i < (long)num_groups * (n / 8); i++)
        if ((uint32_t)qzeros[i] != 0x77777777u) { symmetric = false; break; }

    out->k = k; out->n = n; out->n64 = n64; out->G = G; out->symmetric = symmetric;
    out->qw.assign(w4_qw_words(n64, G), 0);
    out->sc.assign(w4_sc_elems(n64, G), 0);
    if (!symmetric) out->zp.assign(w4_sc_elems(n64, G), f32_to_f16_bits(8.0f));
    else out->zp.clear();
    out->perm = perm;

    auto src_k = [&](int kk) { return use_perm ? perm[kk] : kk; };
    for (int st = 0; st < n64; st++)
        for (int g = 0; g < G; g++) {
            for (int nt = 0; nt < 4; nt++)
                for (int lane = 0; lane < 64; lane++) {
                    int a = lane >> 4, b = lane & 15;
                    int np = st * 64 + nt * 16 + b;          // packed column
                    int col = np < n ? (col_perm ? col_perm[np] : np) : -1;
                    uint32_t dw[4] = {0, 0, 0, 0};
                    for (int s = 0; s < 4; s++)
                        for (int j = 0; j < 8; j++) {
                            int kk = src_k(g * 128 + 32 * s + 8 * a + j);
                            // padded columns decode to q − zero = 0 (zero point 8 when symmetric)
                            uint32_t q = col < 0 ? 8u
                                                 : (((uint32_t)qweight[(long)(kk / 8) * n + col] >> (4 * (kk % 8))) & 0xFu);
                            int d = 2 * (s >> 1) + (j >> 2);
                            dw[d] |= q << (4 * nibble_slot(s & 1, j & 3));
                        }
                    for (int d = 0; d < 4; d++)
                        out->qw[((((size_t)st * G + g) * 4 + nt) * 64 + lane) * 4 + d] = dw[d];
                }
            for (int b = 0; b < 16; b++)
                for (int nt = 0; nt < 4; nt++) {
                    int np = st * 64 + nt * 16 + b;
                    int col = np < n ? (col_perm ? col_perm[np] : np) : -1;
                    size_t idx = (((size_t)st * G + g) * 16 + b) * 4 + nt;
                    if (col < 0) { out->sc[idx] = 0; continue; }
                    int kk0 = src_k(g * 128);
                    int grp = g_idx ? g_idx[kk0] : kk0 / group_size;
                    out->sc[idx] = f32_to_f16_bits(scales[(long)grp * n + col]);
                    if (!symmetric) {
                        uint32_t zw = (uint32_t)qzeros[(long)grp * (n / 8) + col / 8];
                        int zero = (int)((zw >> (4 * (col % 8))) & 0xF) + 1;
                        out->zp[idx] = f32_to_f16_bits((float)zero);
                    }
                }
        }
    return 0;
}

}  // namespace fh
