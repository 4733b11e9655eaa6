// Ingest kernels of the matcher forward (forward.hip), shared with the training forward (train.hip).
#pragma once
#include "common.h"

namespace e2emv {

struct IngestParams {
    const float* kpts[E2EMV_MAX_TUPLE];
    const float* ksc[E2EMV_MAX_TUPLE];
    const void* desc[E2EMV_MAX_TUPLE];
    float img_w[E2EMV_MAX_TUPLE], img_h[E2EMV_MAX_TUPLE];
    int B, T, n_rows, D, c0, f16;
    int Nimg[E2EMV_MAX_TUPLE];  // keypoints of image t
    const float* w0;
    const float* b0;
    float* x0;
    float* h0;
    float* inp;  // optional [img][n_rows][4]: the normalised (x, y, score, 0) the encoder sees (training tape)
};

// [B][D][N] (N contiguous) -> [img][n_rows][D] (D contiguous); rows >= N := 0
__global__ void ingest_transpose(IngestParams p);
// keypoint normalisation + kenc layer 0 (3 -> c0, BN folded, ReLU); rows >= N := 0
__global__ void ingest_kenc0(IngestParams p);

// kenc_fused.hip: layers 1..4 of the keypoint encoder {3, 32, 64, 128, 256, 256}, the descriptor residual and the plane conversion
// of x in ONE launch, bit for bit what ingest_transpose + the four GEMMs + to_planes_exp_kernel make.  in = the inputs as
// ingest_kenc0 took them: in.h0 [n_img * n_rows][32] holds its output, the descriptors are read from in.desc (x0 / inp unused);
// kenc = layers 1..4 (fp32 weights for the first two, fp16 x 2 planes `wh` for the wide ones); outputs: x as scaled planes
// [n_img * n_rows][D], its tile exponents e_x and block maxima a_x [rows / 64][D / 64].
int launch_kenc_fused(e2emv_ctx* ctx, const IngestParams& in, const DenseWeights* kenc, uint16_t* xp, int* e_x, float* a_x, hipStream_t s);

}  // namespace e2emv
