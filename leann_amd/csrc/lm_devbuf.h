// lm_devbuf.h -- DevBuf<T>: a device buffer that belongs to its holder and only ever grows (host code of lm_search.hip's translation unit).
#pragma once
#include <algorithm>

#include "lm_internal.h"

namespace lm {

template <typename T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;  // elements

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;  // (no move either: a declared copy constructor suppresses it)
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }  // on the current device: the holder selects the buffer's device first (lm_index_free)
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Room for `count` elements.  An allocation (the first one, or a growth) takes max(count, min_count, 1) elements, so get() is not NULL after
    // LM_OK.  It frees before it allocates: the contents are lost, and a failure leaves the buffer empty.
    int reserve(size_t count, size_t min_count = 0) {
        if (p_ && count <= cap_) return LM_OK;
        release();
        const size_t n = std::max({count, min_count, (size_t)1});
        void* v = nullptr;
        LM_HIP(hipMalloc(&v, n * sizeof(T)));
        p_ = (T*)v;
        cap_ = n;
        return LM_OK;
    }
};

}  // namespace lm
