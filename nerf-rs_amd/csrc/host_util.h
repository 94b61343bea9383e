// host_util.h -- host-side pieces around the hot path: tensor-directory loader, weight packer, camera,
// minimal JSON reader, PPM writer.  Internal to libnerf_mi355x.so.
#pragma once
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/nerf_mi355x.h"

namespace nerfhost {

struct Tensor {
    std::vector<int64_t> dims;
    std::vector<float> data;
};

// The 12 layers of one network, by the reference's tensor names (src/lib.rs:133-169).
struct HostNet {
    struct L {
        int K = 0, N = 0;
        std::vector<float> w, b;
    };
    L dense[8], bottleneck, viewdirs, rgb, alpha;
};

// load_shapes + load_tensor (src/lib.rs:34-42, 62-74).  Returns NERF_OK or an error code + message.
int read_tensor_dir(const std::string &dir, std::map<std::string, Tensor> &out, std::string &err);
// take_matrix/take_bias by name (src/lib.rs:115-169) + architecture check for the fused kernel.
int assemble_net(std::map<std::string, Tensor> &params, HostNet &net, std::string &err);

// Packed device images (mlp_layout.h).
void pack_network(const HostNet &net, std::vector<float> &wstream, std::vector<float> &small);
// The image the f32 kernels read (mlp_layout.h kChunksFullFolded): the activation-free bottleneck folded into the viewdirs layer,
// formed from pack_network's output with fp64 accumulation.  false if the input does not have the packed image's sizes.
bool fold_network(const std::vector<float> &wstream, const std::vector<float> &small, std::vector<float> &folded_wstream,
                  std::vector<float> &folded_small);
// true iff every value of an f32 device image (stream + small block) is finite: the condition under which the f32 kernels may skip
// k-steps whose ReLU inputs are all zero (fma(a, 0, c) = c needs a finite a; a NaN bias must take the dense path's quieting too)
bool zero_skip_safe(const std::vector<float> &wstream, const std::vector<float> &small);
uint16_t f32_to_bf16_rne(float v);
// f32 by three-way bf16 split (mlp_kernel_bf16x3.hip): w = w1 + w2 + w3
void split_bf16x3(float v, uint16_t out[3]);
// f32 by two-way f16 split (mlp_kernel_f16x2.hip): w = w1 + w2
void split_f16x2(float v, uint16_t out[2]);
// The four 16-bit weight streams of a network (layouts: mlp_layout.h), each the same weights in the arithmetic's element type and piece order.
// The two f16 streams are EMPTY if a weight lies outside the f16 range: that arithmetic is then unavailable for the network.
struct NetStreams {
    std::vector<uint16_t> bf16v2; // mlp_kernel_bf16v2.hip: one bf16 per weight (round-to-nearest-even), output-tile-major
    std::vector<uint16_t> f16v2;  // mlp_kernel_f16v2.hip (certify_zero's pre-filter): its f16 twin, the same order
    std::vector<uint16_t> x3;     // mlp_kernel_bf16x3.hip: three bf16 parts per weight
    std::vector<uint16_t> x2;     // mlp_kernel_f16x2.hip: two f16 parts per weight
};
// All four from the packed f32 image (pack_network's stream or a blob's): every loader calls this.  false if the image has the wrong size.
bool build_streams(const std::vector<float> &packed_ws, NetStreams &out);

// camera_from_samples (src/lib.rs:614-645)
void camera_from_values(float near_, float far_, const float origin[3], const float forward[3], const float up[3],
                        const float hwf[3], int width, int height, nerf_camera *out);
int camera_from_json(const std::string &path, int width, int height, nerf_camera *out, std::string &err);
// Orthonormal basis + slopes of Camera::get_ray_dir (src/lib.rs:216-218, 225-226)
void camera_basis(const nerf_camera &cam, float r[3], float u[3], float f[3], float *sx, float *sy);

void quantize_rgb8(const float *rgb, size_t n_pixels, uint8_t *out);

// nerf_host_api.cpp: error message of context-free calls (nerf_last_error(NULL)), per thread; the packed-blob reader
int fail_noctx(int code, const std::string &msg);
const char *last_error_noctx();
int read_blob_file(const std::string &path, std::vector<float> &wstream, std::vector<float> &small, std::string &err);
int save_ppm(const std::string &path, int width, int height, const float *rgb, std::string &err);
// 1-channel PFM ("Pf", little-endian, rows bottom-up) of a top-row-first map
int save_pfm(const std::string &path, int width, int height, const float *values, std::string &err);
// PAM (P7, RGB_ALPHA, MAXVAL 255) of height x width x 4 bytes
int save_pam(const std::string &path, int width, int height, const uint8_t *rgba, std::string &err);
// binary little-endian PLY of an indexed triangle mesh; normals / rgb (written as uchar through quantize_rgb8) may be NULL
int save_ply(const std::string &path, size_t n_vertices, const float *vertices, const float *normals, const float *rgb, size_t n_triangles,
             const uint32_t *triangles, std::string &err);

// certify_zero's audit policy (nerf_render.cpp render_device; exposed host-only as nerf_debug_certify_policy so that it is tested without a
// GPU).  Given what the audit of one network found in one frame, decide whether the frame stands and, if not, the widened margin:
//   a violation (an audited certificate with a positive exact density)              -> max(4 m, 4 err)
//   least headroom below m / 2 (an audited sample closer to a positive density)     -> max(2 m, 4 err)
//   largest |bf16 - exact| on an audited certificate above m / 2                    -> max(1.25 m, 3 err)
// err = max(largest error, m - least headroom).  Returns 0 (stands), 1 / 2 / 3 (which rule widened; *new_margin is set).
int certify_policy(float margin, uint64_t audited, uint64_t violations, float headroom, float max_error, float *new_margin);

} // namespace nerfhost
