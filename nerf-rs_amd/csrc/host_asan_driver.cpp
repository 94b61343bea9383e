// host_asan_driver.cpp -- drives the HOST-ONLY entry points of the C ABI (nerf_host_api.cpp + host_util.cpp) in a plain g++ build with
// AddressSanitizer + UndefinedBehaviorSanitizer (`make host-asan`; GPU ASan is not available on this pool, and none of this code
// touches the device).  tests/test_host_asan.py feeds it valid, truncated, oversized and malformed weight directories, blobs and
// camera JSON files: every call must come back with a status code and a message -- a sanitizer report aborts with a non-zero exit.
//   host_asan_driver check_dir <dir> | pack_dir <dir> <blob> | check_blob <blob> | camera_json <json> <w> <h> |
//                    debug_pack <dir> | debug_fold <dir> | streams_dir <dir> | quantize | save_ppm <path> <w> <h> | save_pfm <path> <w> <h> | save_pam <path> <w> <h> | split |
//                    ply <path> <n_vertices> <n_triangles> <normals 0|1> <colours 0|1> | stage_layout
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/nerf_mi355x.h"
#include "host_util.h"
#include "stage_layout.h"

static int report(const char *what, int rc) {
    printf("%s rc=%d msg=%s\n", what, rc, rc ? nerfhost::last_error_noctx() : "");
    return 0; // an error CODE is a correct answer; only a crash / sanitizer report fails the run
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "check_dir" && argc == 3) return report("check_dir", nerf_check_network_dir(argv[2]));
    if (cmd == "pack_dir" && argc == 4) return report("pack_dir", nerf_pack_network_dir(argv[2], argv[3]));
    if (cmd == "check_blob" && argc == 3) return report("check_blob", nerf_check_network_blob(argv[2]));
    if (cmd == "camera_json" && argc == 5) {
        nerf_camera cam;
        memset(&cam, 0, sizeof cam);
        const int rc = nerf_camera_from_json(argv[2], atoi(argv[3]), atoi(argv[4]), &cam);
        if (!rc) printf("camera %d %d %.9g %.9g near %.9g far %.9g\n", cam.nx, cam.ny, cam.alpha_width, cam.alpha_height, cam.near_, cam.far_);
        return report("camera_json", rc);
    }
    if (cmd == "debug_pack" && argc == 3) {
        size_t nw = 0, ns = 0;
        int rc = nerf_debug_pack_network_dir(argv[2], nullptr, 0, nullptr, 0, &nw, &ns);
        if (!rc) {
            std::vector<float> ws(nw), sm(ns);
            rc = nerf_debug_pack_network_dir(argv[2], ws.data(), ws.size(), sm.data(), sm.size(), &nw, &ns);
            if (!rc) rc = nerf_debug_pack_network_dir(argv[2], ws.data(), ws.size() - 1, sm.data(), sm.size(), &nw, &ns) == NERF_ERR_INVALID ? 0 : 99; // short buffer refused
            double s = 0; for (float v : ws) s += v; for (float v : sm) s += v;
            printf("packed %zu + %zu floats, sum %.6f\n", nw, ns, s);
        }
        return report("debug_pack", rc);
    }
    if (cmd == "debug_fold" && argc == 3) { // the folded image of the f32 kernels (host_util.cpp fold_network)
        size_t nw = 0, ns = 0;
        int rc = nerf_debug_fold_network_dir(argv[2], nullptr, 0, nullptr, 0, &nw, &ns);
        if (!rc) {
            std::vector<float> ws(nw), sm(ns);
            rc = nerf_debug_fold_network_dir(argv[2], ws.data(), ws.size(), sm.data(), sm.size(), &nw, &ns);
            if (!rc) rc = nerf_debug_fold_network_dir(argv[2], ws.data(), ws.size(), sm.data(), sm.size() - 1, &nw, &ns) == NERF_ERR_INVALID ? 0 : 99; // short buffer refused
            double s = 0; for (float v : ws) s += v; for (float v : sm) s += v;
            printf("folded %zu + %zu floats, sum %.6f\n", nw, ns, s);
        }
        return report("debug_fold", rc);
    }
    if (cmd == "streams_dir" && argc == 3) { // the four 16-bit streams (host_util.cpp build_streams), each into a buffer of exactly its length
        int rc = 0;
        for (int kind = NERF_STREAM_BF16V2; kind <= NERF_STREAM_F16X2 && !rc; ++kind) {
            size_t n = 0;
            int available = -1;
            rc = nerf_debug_network_stream_dir(argv[2], kind, nullptr, 0, &n, &available);
            if (rc) break;
            std::vector<uint16_t> s(n);
            rc = nerf_debug_network_stream_dir(argv[2], kind, s.data(), s.size(), &n, &available);
            if (!rc && n && nerf_debug_network_stream_dir(argv[2], kind, s.data(), n - 1, &n, &available) != NERF_ERR_INVALID) rc = 99; // short buffer refused
            if (!rc && available != (n ? 1 : 0)) rc = 98;
            unsigned long long sum = 0; for (uint16_t v : s) sum += v;
            printf("stream %d: %zu elements, available %d, sum %llu\n", kind, n, available, sum);
        }
        if (!rc && nerf_debug_network_stream_dir(argv[2], 4, nullptr, 0, nullptr, nullptr) != NERF_ERR_INVALID) rc = 97;
        return report("streams_dir", rc);
    }
    if (cmd == "quantize") { // clamp + NaN/inf through the quantisers (src/lib.rs:573-577, :582-592)
        const float v[] = {-1.f, 0.f, 0.5f, 1.f, 2.f, NAN, INFINITY, -INFINITY, 1e-9f, 0.999999f, 0.25f, 0.75f};
        uint8_t a[12], b[16];
        nerf_quantize_rgb8(v, 4, a);
        nerf_quantize_rgba8(v, 4, b);
        for (int i = 0; i < 12; ++i) printf("%d ", a[i]);
        printf("| ");
        for (int i = 0; i < 16; ++i) printf("%d ", b[i]);
        printf("\n");
        nerf_quantize_rgb8(v, 0, a);
        return report("quantize", 0);
    }
    if (cmd == "save_ppm" && argc == 5) {
        const int w = atoi(argv[3]), h = atoi(argv[4]);
        std::vector<float> img(w > 0 && h > 0 ? (size_t)w * h * 3 : 0);
        for (size_t i = 0; i < img.size(); ++i) img[i] = (float)(i % 97) / 96.f - 0.01f;
        return report("save_ppm", nerf_save_ppm(argv[2], w, h, img.data()));
    }
    if (cmd == "save_pfm" && argc == 5) {
        const int w = atoi(argv[3]), h = atoi(argv[4]);
        std::vector<float> m(w > 0 && h > 0 ? (size_t)w * h : 0);
        for (size_t i = 0; i < m.size(); ++i) m[i] = (float)(i % 89) * 0.0625f - 1.5f;
        return report("save_pfm", nerf_save_pfm(argv[2], w, h, m.data()));
    }
    if (cmd == "save_pam" && argc == 5) { // the buffer is exactly w x h x 4 bytes: an over-read is a report (1 x 1 included)
        const int w = atoi(argv[3]), h = atoi(argv[4]);
        std::vector<uint8_t> px(w > 0 && h > 0 ? (size_t)w * h * 4 : 0);
        for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 37u + 11u);
        int rc = nerf_save_pam(argv[2], w, h, px.data());
        if (!rc) { // read it back: header + bytes, nothing more
            const std::string hdr = "P7\nWIDTH " + std::to_string(w) + "\nHEIGHT " + std::to_string(h) + "\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n";
            std::vector<char> got(hdr.size() + px.size() + 1);
            FILE *f = fopen(argv[2], "rb");
            const size_t n = f ? fread(got.data(), 1, got.size(), f) : 0;
            if (f) fclose(f);
            if (n != hdr.size() + px.size() || memcmp(got.data(), hdr.data(), hdr.size()) || memcmp(got.data() + hdr.size(), px.data(), px.size())) rc = 99;
        }
        return report("save_pam", rc);
    }
    if (cmd == "ply" && argc == 7) { // the arrays are exactly as long as the counts say: an over-read is a report (zero counts included)
        const long long nv = atoll(argv[3]), nt = atoll(argv[4]);
        const bool with_n = atoi(argv[5]) != 0, with_c = atoi(argv[6]) != 0;
        if (nv < 0 || nt < 0 || nv > 1000000 || nt > 1000000) return 2;
        std::vector<float> v(3 * (size_t)nv), n(with_n ? (nv ? 3 * (size_t)nv : 1) : 0), c(with_c ? (nv ? 3 * (size_t)nv : 1) : 0); // non-NULL also for no vertices
        std::vector<uint32_t> t(3 * (size_t)nt);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (float)(i % 101) * 0.03125f - 1.5f;
        for (size_t i = 0; i < n.size(); ++i) n[i] = (float)(i % 7) - 3.0f;
        for (size_t i = 0; i < c.size(); ++i) c[i] = i % 13 == 0 ? NAN : (float)(i % 19) / 16.f - 0.1f; // below 0, above 1 and NaN go through the quantiser
        for (size_t i = 0; i < t.size(); ++i) t[i] = nv ? (uint32_t)((i * 7u + 3u) % (size_t)nv) : 0u;
        int rc = nerf_save_ply(argv[2], (size_t)nv, nv ? v.data() : nullptr, with_n ? n.data() : nullptr, with_c ? c.data() : nullptr, (size_t)nt,
                               nt ? t.data() : nullptr);
        if (!rc) { // read it back: header + records, nothing more
            std::string hdr = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(nv) + "\nproperty float x\nproperty float y\nproperty float z\n";
            if (with_n) hdr += "property float nx\nproperty float ny\nproperty float nz\n";
            if (with_c) hdr += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
            hdr += "element face " + std::to_string(nt) + "\nproperty list uchar uint vertex_indices\nend_header\n";
            const size_t vrec = 12 + (with_n ? 12 : 0) + (with_c ? 3 : 0), body = (size_t)nv * vrec + (size_t)nt * 13;
            std::vector<char> got(hdr.size() + body + 1);
            FILE *f = fopen(argv[2], "rb");
            const size_t m = f ? fread(got.data(), 1, got.size(), f) : 0;
            if (f) fclose(f);
            if (m != hdr.size() + body || memcmp(got.data(), hdr.data(), hdr.size())) rc = 99;
            if (!rc && nv && memcmp(got.data() + hdr.size(), v.data(), 12)) rc = 98;
            if (!rc && nt && (got[hdr.size() + (size_t)nv * vrec] != 3 || memcmp(got.data() + hdr.size() + (size_t)nv * vrec + 1, t.data(), 12))) rc = 97;
        }
        if (!rc && nv && nt) { // an index beyond the vertices, a missing array: refused, nothing crashes
            t[t.size() - 1] = (uint32_t)nv;
            if (nerf_save_ply(argv[2], (size_t)nv, v.data(), nullptr, nullptr, (size_t)nt, t.data()) != NERF_ERR_INVALID) rc = 96;
            if (nerf_save_ply(argv[2], (size_t)nv, nullptr, nullptr, nullptr, 0, nullptr) != NERF_ERR_INVALID) rc = 95;
            if (nerf_save_ply(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) != NERF_ERR_INVALID) rc = 94;
        }
        return report("ply", rc);
    }
    if (cmd == "split") {
        const float v[] = {0.f, -0.f, 1.f, -3.14159274f, 65504.f, 7e4f, 1e-8f, 6e-8f, 1e30f, -1e-30f, NAN, INFINITY};
        uint16_t p3[3 * 12], p2[2 * 12];
        int rc = nerf_debug_split_bf16x3(v, 12, p3);
        if (!rc) rc = nerf_debug_split_f16x2(v, 12, p2);
        if (!rc) rc = nerf_debug_split_f16x2(nullptr, 0, nullptr);
        for (int i = 0; i < 36; ++i) printf("%04x ", p3[i]);
        printf("| ");
        for (int i = 0; i < 24; ++i) printf("%04x ", p2[i]);
        printf("\n");
        return report("split", rc);
    }
    if (cmd == "stage_layout") { // the bump allocator behind every staging layout and pass workspace (stage_layout.h); rc = the first failed check
        using nerfint::StageLayout;
        const size_t A = StageLayout::kAlign;
        int rc = 0;
        std::vector<char> base(8 * A);
        float src[3] = {1.f, 2.f, 3.f}, dst[5];
        StageLayout l;
        const int up = l.add(sizeof(float), 3, src);                     // 12 bytes: the next part starts one alignment unit later
        const int absent = l.opt(false, sizeof(float), 1000, src, dst);  // an absent part: no space, no copy, no address
        const int present = l.opt(true, sizeof(float), 5, nullptr, dst);
        const int empty = l.add(sizeof(float), 0, src, dst);             // a zero-length part: an address, no bytes
        const int guarded = l.add(4, 32 + 70 + 32, nullptr, dst, 0xFF);  // guard words, list, guard words: ONE part, contiguous
        const int last = l.add(1, A + 1, nullptr, nullptr, 0x00);
        if (l.refused || l.n_parts != 5 || absent != StageLayout::kAbsent || up != 0 || present != 1 || last != 4) rc = 1;
        if (!rc && l.at<char>(base.data(), absent) != nullptr) rc = 2;
        for (int k = 0; k < l.n_parts && !rc; ++k)
            if (l.parts[k].offset % A || l.at<char>(base.data(), k) != base.data() + l.parts[k].offset) rc = 3;
        if (!rc && (l.parts[present].offset != A || l.parts[empty].offset != 2 * A || l.parts[empty].bytes != 0 || l.parts[guarded].offset != 2 * A)) rc = 4;
        if (!rc && (l.parts[guarded].bytes != 4 * 134 || l.parts[last].offset != 2 * A + 3 * A || l.total != 5 * A + 2 * A || l.total > base.size())) rc = 5;
        if (!rc && (l.parts[up].upload != src || l.parts[up].download || l.parts[up].fill != StageLayout::kNoFill || l.parts[present].download != dst ||
                    l.parts[guarded].fill != 0xFF || l.parts[last].fill != 0x00)) rc = 6;
        for (int k = 0; k < l.n_parts && !rc; ++k) { // every part lies inside the total, and a fill of each stays inside the buffer
            if (l.parts[k].offset + l.parts[k].bytes > l.total) rc = 7;
            else if (l.parts[k].fill != StageLayout::kNoFill) memset(l.at<char>(base.data(), k), l.parts[k].fill, l.parts[k].bytes);
        }
        // sizes that would overflow size_t are refused, not wrapped: elem * count, the padding of one part, the running total
        StageLayout o1, o2, o3;
        if (!rc && (o1.add(8, SIZE_MAX / 4) != StageLayout::kAbsent || !o1.refused)) rc = 8;
        if (!rc && (o2.add(1, SIZE_MAX - 3) != StageLayout::kAbsent || !o2.refused)) rc = 9;
        if (!rc && (o3.add(1, SIZE_MAX / 2) < 0 || o3.add(1, SIZE_MAX / 2) != StageLayout::kAbsent || !o3.refused)) rc = 10;
        if (!rc && o3.add(1, 1) != StageLayout::kAbsent) rc = 11; // a refused layout stays refused
        StageLayout many;                                          // more parts than the table holds: refused as well
        for (int k = 0; k < StageLayout::kMaxParts; ++k) if (many.add(4, 1) != k) rc = rc ? rc : 12;
        if (!rc && (many.add(4, 1) != StageLayout::kAbsent || !many.refused)) rc = 13;
        printf("stage_layout total %zu parts %d\n", l.total, l.n_parts);
        if (rc) nerfhost::fail_noctx(rc, "stage_layout: check failed");
        return report("stage_layout", rc);
    }
    fprintf(stderr, "usage: see the header comment\n");
    return 2;
}
