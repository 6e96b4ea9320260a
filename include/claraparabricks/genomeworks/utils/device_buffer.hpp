// Minimal device_buffer<T> (reference
// common/base/include/claraparabricks/genomeworks/utils/device_buffer.hpp):
// the data() / size() surface that call sites of cudamapper's Index and
// Matcher use.  Here it is a view of device memory owned by the object that
// returns it (the index or the matcher), valid for that object's lifetime.
#pragma once

#include <cstddef>

namespace claraparabricks
{
namespace genomeworks
{

template <typename T>
class device_buffer
{
public:
    using value_type = T;
    using size_type  = std::ptrdiff_t;

    device_buffer() = default;
    device_buffer(T* data, size_type size)
        : data_(data)
        , size_(size)
    {
    }
    T* data() { return data_; }
    const T* data() const { return data_; }
    size_type size() const { return size_; }
    T* begin() { return data_; }
    const T* begin() const { return data_; }
    T* end() { return data_ + size_; }
    const T* end() const { return data_ + size_; }

private:
    T* data_        = nullptr;
    size_type size_ = 0;
};

} // namespace genomeworks
} // namespace claraparabricks
