// Copy yardsticks of tools/layernorm_bench.py: kernels that move the bytes a ViT-block LayerNorm moves per element and compute nothing.
//   mix 1 (LN1: delta, keep_x):        reads x fp32 + delta fp16, writes y fp16                          (4 + 2 | 2 B per element)
//   mix 2 (LN2: delta, delta2, store): reads x fp32 + delta fp16 + delta2 fp16, writes x fp32 + y fp16   (4 + 2 + 2 | 4 + 2 B per element)
// Same stream count, widths (16-B fp32 and 8-B fp16 accesses per lane) and nontemporal hints as the LayerNorm kernels; the outputs are
// bit mixes of the inputs so that no load can be dropped.  Every thread issues the loads of UNROLL groups before its first store.  The rate
// these reach is what the device grants this access pattern: the bound the LayerNorm kernels are judged against.
//   hipcc -O3 --offload-arch=gfx950 -shared -fPIC tools/layernorm_copy.hip -o tools/liblayernorm_copy.so   (layernorm_bench.py does it)
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int MIX, int UNROLL>
__global__ __launch_bounds__(256) void ln_copy_kernel(u32x4* __restrict__ x, const u32x2* __restrict__ d, const u32x2* __restrict__ d2,
                                                      u32x2* __restrict__ y, int64_t groups) {
    const int64_t base = (int64_t)blockIdx.x * (256 * UNROLL) + threadIdx.x;
    u32x4 xv[UNROLL];
    u32x2 dv[UNROLL], ev[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + u * 256;
        if (i < groups) {
            xv[u] = __builtin_nontemporal_load(x + i);
            dv[u] = __builtin_nontemporal_load(d + i);
            if (MIX == 2) ev[u] = __builtin_nontemporal_load(d2 + i);
        }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int64_t i = base + u * 256;
        if (i < groups) {
            u32x2 o = u32x2{dv[u][0] ^ xv[u][0] ^ xv[u][1], dv[u][1] ^ xv[u][2] ^ xv[u][3]};
            if (MIX == 2) {
                o ^= ev[u];
                __builtin_nontemporal_store(u32x4{xv[u][0] ^ ev[u][0], xv[u][1], xv[u][2] ^ ev[u][1], xv[u][3]}, x + i);
            }
            y[i] = o;
        }
    }
}

template <int UNROLL>
static int ln_copy_launch(int mix, void* x, const void* d, const void* d2, void* y, int64_t groups, hipStream_t stream) {
    const dim3 grid((unsigned)((groups + 256 * UNROLL - 1) / (256 * UNROLL)));
    if (mix == 1) hipLaunchKernelGGL((ln_copy_kernel<1, UNROLL>), grid, dim3(256), 0, stream, (u32x4*)x, (const u32x2*)d, (const u32x2*)d2, (u32x2*)y, groups);
    else hipLaunchKernelGGL((ln_copy_kernel<2, UNROLL>), grid, dim3(256), 0, stream, (u32x4*)x, (const u32x2*)d, (const u32x2*)d2, (u32x2*)y, groups);
    return (int)hipGetLastError();
}

// elements = rows * D (a multiple of 4; dense rows); unroll = 1, 2 or 4 groups of 4 elements per thread.  Returns the hipError_t of the launch.
extern "C" int ln_copy(int mix, int unroll, void* x, const void* d, const void* d2, void* y, int64_t elements, void* stream) {
    if ((mix != 1 && mix != 2) || elements <= 0 || (elements & 3)) return (int)hipErrorInvalidValue;
    const int64_t groups = elements >> 2;
    if (unroll == 1) return ln_copy_launch<1>(mix, x, d, d2, y, groups, (hipStream_t)stream);
    if (unroll == 2) return ln_copy_launch<2>(mix, x, d, d2, y, groups, (hipStream_t)stream);
    if (unroll == 4) return ln_copy_launch<4>(mix, x, d, d2, y, groups, (hipStream_t)stream);
    return (int)hipErrorInvalidValue;
}
