/*
 * util.h -- small helpers, counterpart of
 * /root/reference/InstanceStixels/include/InstanceStixels/util.h:22-48.  The reference's
 * CUDA_CHECK_RETURN prints and exit(1)s on a runtime failure (util.h:34-42); IS_CHECK_RETURN
 * keeps that error convention for the C-ABI return codes of the HIP core.
 */
#ifndef INSTANCESTIXELS_AMD_UTIL_H_
#define INSTANCESTIXELS_AMD_UTIL_H_

#include <cstddef>
#include <cstdlib>
#include <iostream>
#include <utility>

#include "instance_stixels_core.h"

constexpr int WAVEFRONT_SIZE = 64; /* the reference's WARP_SIZE = 32 has no meaning on CDNA */

#define IS_CHECK_RETURN(value) IsCheckReturnAux(__FILE__, __LINE__, #value, (value))

static inline void IsCheckReturnAux(const char* file, unsigned line, const char* statement,
                                    int rc) {
    if (rc == IS_OK) return;
    std::cerr << statement << " returned " << is_last_error() << "(" << rc << ") at " << file
              << ":" << line << std::endl;
    std::exit(1);
}

static inline int divUp(int total, int grain) { return (total + grain - 1) / grain; }

/* One device (is_device_malloc) or pinned host (is_host_malloc) block of T, with its capacity in elements.
 * reserve(n) replaces a smaller block by a new one of n elements (contents are not kept); release() frees it.
 * The destructor frees NOTHING: the owning classes release in Finish(), like the reference, and a free during
 * static destruction can run after the HIP runtime has shut down. */
template <typename T, bool Pinned>
class IsArray {
public:
    IsArray() = default;
    IsArray(const IsArray&) = delete;
    IsArray& operator=(const IsArray&) = delete;
    IsArray(IsArray&& o) noexcept : m_ptr(std::exchange(o.m_ptr, nullptr)), m_cap(std::exchange(o.m_cap, 0)) {}
    IsArray& operator=(IsArray&& o) noexcept { std::swap(m_ptr, o.m_ptr); std::swap(m_cap, o.m_cap); return *this; }
    T* get() const { return m_ptr; }
    size_t capacity() const { return m_cap; }
    void reserve(size_t n) {
        if (n <= m_cap) return;
        void* p = nullptr;
        IS_CHECK_RETURN(Pinned ? is_host_malloc(&p, n * sizeof(T)) : is_device_malloc(&p, n * sizeof(T)));
        release();
        m_ptr = static_cast<T*>(p);
        m_cap = n;
    }
    void release() {
        if (m_ptr) IS_CHECK_RETURN(Pinned ? is_host_free(m_ptr) : is_device_free(m_ptr));
        m_ptr = nullptr;
        m_cap = 0;
    }

private:
    T* m_ptr = nullptr;
    size_t m_cap = 0;
};
template <typename T> using DeviceArray = IsArray<T, false>;
template <typename T> using PinnedArray = IsArray<T, true>;

#endif
