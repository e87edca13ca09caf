// vapor_image.h - what the HIP-free host plans of a call share (vapor_polish_call.h, vapor_seqset_plan.h, the trace entry in
// vapor_hip.hip): why a call is refused, and an upload image whose tables have their places stated once.  No HIP.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vapor_image {

// why a call is refused: the code and the message (a plan says whether its messages carry the entry's name or the entry prepends it)
struct Refusal {
    int code = 0;
    const char* msg = nullptr;
    explicit operator bool() const { return code != 0; }
};

// A table of an upload image: n entries of T from byte `off` on.  The image is carved once; the host fills a table and the
// launches take its entries through in(), given the host's or the device's copy of the image.  A table the call does not have
// takes no room.
template <typename T>
struct Table {
    size_t off = 0, n = 0;
    T* in(uint8_t* image) const { return reinterpret_cast<T*>(image + off); }
    const T* in(const uint8_t* image) const { return reinterpret_cast<const T*>(image + off); }
    size_t bytes() const { return sizeof(T) * n; }
    size_t end() const { return off + (bytes() + 7) / 8 * 8; }           // where the next table of a Carve starts
    void fill(std::vector<uint8_t>& image, const std::vector<T>& from) const
    {
        if (n) memcpy(image.data() + off, from.data(), sizeof(T) * n);
    }
};
struct Carve {                     // a running offset, every table starting on 8 bytes; `off` is the image's size once every table is taken
    size_t off = 0;
    template <typename T>
    void take(Table<T>& t, size_t n) { t.off = off; t.n = n; off = t.end(); }
};

}  // namespace vapor_image
