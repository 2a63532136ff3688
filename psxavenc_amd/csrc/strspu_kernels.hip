// strspu_kernels.hip -- the audio sectors of a muxed STRSPU stream on the device for MI355X (gfx950), hand-written HIP: SPU-ADPCM
// unit records into 2048-byte audio chunks ("psxhip STRSPU v1"; the block placement is the SPUI writer's,
// filefmt.c:323-371).  A sector is 128 x 16 bytes: one 128-lane workgroup per sector, one lane per 16 bytes -- lanes 0 and 1 the
// chunk header, lanes 2 .. 127 one SPU block each.  No LDS, no tables: a 16-byte load, selects in registers, four dword stores.
// (Its own file: sector_kernels.hip holds the kernels that need the EDC tables.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_adpcm_internal.h"

namespace {

__global__ __launch_bounds__(128) void strspu_audio_sector_kernel(const psxhip_strspu_job_t job) {
    const int t = (int)threadIdx.x;
    // ---- uniform: the chunk, its place, the options
    const int k = (int)blockIdx.x, K = job.n_sectors;
    const int ch = job.channels;
    const int B = ch == 2 ? 63 : 126;                                  // SPU blocks per channel per sector
    const int d = (job.options & PSXHIP_STRSPU_NO_LEADING_DUMMY) ? 0 : 1;
    const bool loop = (job.options & PSXHIP_STRSPU_LOOP) != 0u;
    const bool last = k == K - 1;
    const int slot = job.dst_sector ? job.dst_sector[k] : k;
    const uint8_t* units = job.units + (size_t)blockIdx.y * job.units_stream_stride;
    uint32_t* dst = (uint32_t*)(job.out + (size_t)blockIdx.y * job.out_stream_stride + (size_t)slot * 2048u) + 4 * t;

    // ---- per lane: block j of the payload is block b of channel c's lane, unit u = k B + b - d of that channel's chain (u < 0: the
    //      leading dummy block).  The header lanes (j < 0) load a record too -- one of the chunk before, or record 0 -- and drop it.
    const int j = t - 2;
    const int c = j >= B ? 1 : 0;
    const int b = j - c * B;
    const int u = k * B + b - d;
    const int rec = (u > 0 ? u : 0) * ch + c;
    const uint4 r = *(const uint4*)(units + (size_t)rec * 16u);
    const bool dummy = u < 0;
    const bool tail = b == B - 1;                                       // the chunk's last block of this channel, filefmt.c:343-358
    const bool trap = tail && !loop && last;
    uint4 v;
    v.x = (dummy || trap) ? 0u : r.x;
    v.y = (dummy || trap) ? 0u : r.y;
    v.z = (dummy || trap) ? 0u : r.z;
    v.w = (dummy || trap) ? 0u : r.w;
    if (tail) v.x = (v.x & 0xFFFF00FFu) | (loop ? 0x0300u : (last ? 0x0500u : (v.x & 0x0000FF00u)));

    // ---- the chunk header: 32 bytes, little endian
    const uint32_t flags = (last ? 1u : 0u) | ((k == 0 && d) ? 2u : 0u) | (loop ? 4u : 0u);
    if (t == 0) {
        v.x = 0x0160u | ((job.options & 0xFFFFu) << 16);               // 60 01, the audio chunk id
        v.y = 0x00010000u;                                             // chunk index 0 of 1
        v.z = (uint32_t)(k + 1);
        v.w = 2016u;
    } else if (t == 1) {
        v.x = (uint32_t)ch | ((uint32_t)(16 * B) << 16);
        v.y = (uint32_t)job.frequency;
        v.z = k == 0 ? 0u : 28u * (uint32_t)(k * B - d);               // the chunk's first sample, per channel
        v.w = flags;
    }
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;           // (d_out is promised 4-byte alignment only)
}
}  // namespace

extern "C" hipError_t psxhip_strspu_audio_sectors_launch(const psxhip_strspu_job_t* j, int n_streams, void* stream) {
    hipLaunchKernelGGL(strspu_audio_sector_kernel, dim3((unsigned)j->n_sectors, (unsigned)n_streams), dim3(128), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
