// bg_u8.h -- what the Background module's uint8 kernels share (bg_io.hip, bg_scene.hip): the byte of a packed group of 4 pixels
// and the one saturating cast from the generator's image to a byte.
#pragma once

__device__ __forceinline__ unsigned byte_of(const unsigned (&w)[3], int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; }

// deprocess + convert_image_dtype(saturate=True): floor(clamp((x + 1) / 2, 0, 1) * 255 + 0.5), clamped to 0..255; every
// operation rounded on its own (no fused y * 255 + 0.5).  fminf / fmaxf drop a NaN operand, so a NaN pixel comes out as 0.
__device__ __forceinline__ unsigned unit_to_u8(float x) {
#pragma clang fp contract(off)
    const float h = (x + 1.f) / 2.f;
    const float y = fminf(fmaxf(h, 0.f), 1.f) * 255.f;
    const float r = y + 0.5f;
    return (unsigned)(int)fminf(fmaxf(floorf(r), 0.f), 255.f);
}
