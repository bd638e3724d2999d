// spk.h -- what the speaker encoder's inference (spk.hip) and training (spk_train.hip) entry points share: the geometry of the
// recurrence, the launch descriptors of the forward kernels, and the host-side handle.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/gradtts_abi.h"

namespace gtts {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int SPK_H = 256;          // hidden size the recurrence kernel is built for
constexpr int SPK_G = 4 * SPK_H;    // gate rows
constexpr int SPK_TILE = 16;        // sequences per workgroup (the MFMA's column count)
constexpr int SPK_WAVES = 8;        // waves per recurrence workgroup; each owns SPK_H / SPK_WAVES = 32 hidden units (8 row tiles)
constexpr int SPK_HS = SPK_H + 4;   // LDS row stride of h in floats: rows 16 bytes apart in the banks
constexpr int SPK_KB = SPK_H / 16;  // 16-wide k blocks of the recurrent product

struct SpkProjArgs {
    const float4 *wih;      // packed fragments [64 tiles][KB][64]
    const float *bias;      // [4H] b_ih + b_hh
    const float *x;         // layer 0: frames [U][T_total][K];  above: hseq [M][K]
    float *G;               // [M][4H]
    int M, T, K, KB;
    int sliced, P, S, T_total;
};

struct SpkRecArgs {
    const float4 *whh;      // packed fragments [16 unit groups][4 gates][SPK_KB][64]
    float *G;               // [N][T][4H]; the training forward leaves the activated gates here
    float *C;               // training forward: c_t [N][T][H]
    float *hseq;            // [N][T][H] or nullptr (last layer at inference)
    float *hlast;           // [N][H] or nullptr
    int N, T;
};

hipError_t spk_launch_proj(const SpkProjArgs &pa, hipStream_t st);
hipError_t spk_launch_rec(const SpkRecArgs &ra, bool save, hipStream_t st);
hipError_t spk_launch_head(const float *hlast, const float *wt, const float *bias, float *embeds, float *raw, int N, int H, int E, hipStream_t st);
bool spk_shape_ok(int N, int T);    // N, T >= 1 and N T 4H below 2^31

}  // namespace gtts

struct SpkParam {
    std::string name;
    int rank;
    int dims[4];
};

// host-side metadata: configuration, state_dict layout, offsets into the packed blob
struct gtts_spk {
    gtts_spk_cfg cfg;
    std::vector<SpkParam> params;
    std::vector<int> kb;                        // k blocks of each layer's input projection
    std::vector<size_t> off_wih, off_whh, off_bias;
    size_t off_lin_wt, off_lin_b, blob_bytes;
};
