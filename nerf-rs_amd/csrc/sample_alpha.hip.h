// sample_alpha.hip.h -- the opacity of one sample and the transmittance cut, as compute_weights has them (src/lib.rs:261-280).  Shared by the
// sampling kernels (sampling_kernels.hip sample_alpha: what k_resample and k_composite weigh their samples with) and the cut of the sigma-only
// sampling launch (mlp_kernel.hip), which must find the resampler's cut from the same inputs with the same operations in the same order.
#pragma once
#include <hip/hip_runtime.h>

// t_end: the next sample's t, or the ray's far behind the last sample
__device__ __forceinline__ float sample_alpha_of(float t_cur, float t_end, float sigma) {
    float delta = t_end - t_cur;
    if (delta < 0.0f) delta = 0.0f;
    return 1.0f - expf(-sigma * delta);
}

// one sample of weights_scan's walk (sampling_kernels.hip): T behind the sample, frozen once the ray is cut (src/lib.rs:273-279)
__device__ __forceinline__ void transmittance_step(float &T, bool &cut, float alpha) {
    T = cut ? T : T * (1.0f - alpha);
    cut = cut || T < 1e-4f;
}
