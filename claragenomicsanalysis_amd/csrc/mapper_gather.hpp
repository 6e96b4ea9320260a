// What the byte movers share (device translation units only):
// gather_overlap_regions_kernel (mapper_gather.hip) and gather_poa_slices_kernel
// (polish_gather.hip).  Both cut a destination [A, A + len) into the 16-byte
// chunks of the buffer's own alignment, store whole chunks as one aligned
// 16-byte vector and write the chunks that stick out of the sequence byte by
// byte; both read their source as aligned 32-bit words, so the source arrays
// are padded by kReadsPad (mapper_reads.hpp) at either end.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gwamd
{
namespace mapper
{

constexpr uint32_t kChunk       = 16;
constexpr uint32_t kPieceChunks = 256; // per wave: four steps of 64 lanes

__device__ inline uint32_t uniform(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }

__device__ inline uint8_t complement(uint8_t c)
{
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
}

// 0xff in every byte of v that equals c
__device__ inline uint32_t bytes_equal(uint32_t v, uint32_t c)
{
    const uint32_t x = v ^ (c * 0x01010101u);
    // the high bit of a byte stays clear only when the byte is zero (no carry crosses a byte)
    const uint32_t nonzero = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return ((nonzero ^ 0x80808080u) >> 7) * 0xffu;
}

// complement() of the four bytes of v: 'A' ^ 'T' == 0x15, 'C' ^ 'G' == 0x04
__device__ inline uint32_t complement4(uint32_t v)
{
    const uint32_t at = bytes_equal(v, 'A') | bytes_equal(v, 'T');
    const uint32_t cg = bytes_equal(v, 'C') | bytes_equal(v, 'G');
    return v ^ (at & 0x15151515u) ^ (cg & 0x04040404u);
}

// src[0, 16) for any src, from the five aligned words that hold it
__device__ inline uint4 load16(const uint8_t* src)
{
    const uintptr_t address = reinterpret_cast<uintptr_t>(src);
    const uint32_t* w       = reinterpret_cast<const uint32_t*>(address & ~uintptr_t(3));
    const uint32_t shift    = uint32_t(address & 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    return uint4{__builtin_amdgcn_alignbyte(w1, w0, shift), __builtin_amdgcn_alignbyte(w2, w1, shift),
                 __builtin_amdgcn_alignbyte(w3, w2, shift), __builtin_amdgcn_alignbyte(w4, w3, shift)};
}

// the 16 bytes of v in the opposite order
__device__ inline uint4 reverse16(uint4 v)
{
    return uint4{__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x)};
}

} // namespace mapper
} // namespace gwamd
