// The C ABI's handle of a DefaultDeviceAllocator pool (gwamd_device_allocator,
// include/gwamd_cudaaligner.h), shared by the aligner and the mapper entry points.
#pragma once

#include <claraparabricks/genomeworks/utils/allocator.hpp>

struct gwamd_device_allocator
{
    claraparabricks::genomeworks::DefaultDeviceAllocator alloc;
};
