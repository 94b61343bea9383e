// stage_layout.h -- one bump allocator for everything the host carves out of a single device buffer: the staging of a host-pointer entry
// point (inputs to upload, outputs to download, regions to fill) and the pass workspaces of nerf_render.cpp.  A caller declares its parts
// in order; every part starts on a kAlign-byte boundary; an absent part (opt with wanted == false) occupies nothing and has no address.
// Plain host code without HIP, so that the CPU sanitizer driver can include it; Staging (nerf_internal.h) issues the copies.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nerfint {

struct StageLayout {
    static constexpr size_t kAlign = 256;
    static constexpr int kMaxParts = 16, kAbsent = -1, kNoFill = -1;
    struct Part {
        size_t offset, bytes;
        const void *upload; // host source, or NULL
        void *download;     // host destination, or NULL
        int fill;           // byte to fill the part with before the launches (0x00 / 0xFF), or kNoFill
    };
    Part parts[kMaxParts];
    int n_parts = 0;
    size_t total = 0;
    bool refused = false; // a size overflowed size_t or the parts ran out: total and the offsets mean nothing

    // a part of `count` elements of `elem` bytes -> its index.  A guarded region is ONE part (guards and list stay contiguous).
    int add(size_t elem, size_t count, const void *upload = nullptr, void *download = nullptr, int fill = kNoFill) {
        if (refused) return kAbsent;
        if (n_parts == kMaxParts || (count && elem > SIZE_MAX / count)) { refused = true; return kAbsent; }
        const size_t bytes = elem * count, padded = (bytes + (kAlign - 1)) & ~(kAlign - 1);
        if (padded < bytes || padded > SIZE_MAX - total) { refused = true; return kAbsent; }
        parts[n_parts] = Part{total, bytes, upload, download, fill};
        total += padded;
        return n_parts++;
    }
    // an optional part: kAbsent (no space, no copy, at() == NULL) unless wanted
    int opt(bool wanted, size_t elem, size_t count, const void *upload = nullptr, void *download = nullptr, int fill = kNoFill) {
        return wanted ? add(elem, count, upload, download, fill) : kAbsent;
    }
    template <class T>
    T *at(void *base, int part) const { return part < 0 ? nullptr : (T *)((char *)base + parts[part].offset); }
};

} // namespace nerfint
