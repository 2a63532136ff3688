// strspu_demux_kernels.hip -- the audio half of the STRSPU reader on the device for MI355X (gfx950), hand-written HIP
// (psxhip_strspu_demux_device, psxhip_spu_deinterleave_device; include/psxav_hip.h): the audio chunks of a muxed
// format 8 stream -> SPU unit records in the order one chain per channel reads them, a record per chunk, a summary per stream.  The
// inverse of strspu_audio_sector_kernel (strspu_kernels.hip); the rules are "psxhip STRSPU demux v1", restated sequentially in
// tests/strspu_demux_ref.py.  The video half is the STR reader's (str_demux_kernels.hip) run as format 9 in front of this, on the same
// stream; nothing is read back:
//   init           one thread per stream: the audio summary's start values
//   scan           one thread per sector reads the chunk header (strspu_chunk.h), classifies the sector, takes the owner of its chunk
//                  number by integer atomicMin on a word of its own, counts the sectors per number, rewrites the sector's table entry
//                  and moves the audio count from n_other to n_audio
//   de-interleave  the hot path, shared with psxhip_spu_deinterleave_device: one lane per 16-byte block, consecutive lanes write
//                  consecutive records as whole 16-byte stores; the source side is `channels` contiguous runs per wavefront, read as
//                  16 bytes at once when every block is 16-byte aligned, else as four dwords
//   finish         one thread per chunk number: info, status, the audio summary
// Every index that comes from the stream's bytes -- the chunk number -- is compared with its bound before it addresses memory; the
// owner table holds positions the scan pass took from its own thread index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_internal.h"
#include "psxhip_strspu_demux_internal.h"

namespace {

constexpr int kSector = 2048;

__device__ __forceinline__ const uint32_t* sector_words(const psxhip_strspu_demux_job_t& j, int s, uint32_t pos) {
    return (const uint32_t*)(j.d_sectors + (size_t)s * j.in_stream_stride + (size_t)pos * kSector);
}

__global__ __launch_bounds__(256) void strspu_demux_init_kernel(const psxhip_strspu_demux_job_t j) {
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= j.n_streams) return;
    psxhip_strspu_audio_summary_t a = {0, 0, -1, 0};
    j.d_audio_summary[s] = a;
}

__global__ __launch_bounds__(256) void strspu_demux_scan_kernel(const psxhip_strspu_demux_job_t j) {
    const int tid = (int)threadIdx.x, lane = tid & 63, s = (int)blockIdx.y;
    const int i = (int)blockIdx.x * 256 + tid;
    bool audio = false, dropped = false;
    if (i < j.n_sectors) {
        const uint32_t* w = sector_words(j, s, (uint32_t)i);
        const uint32_t h[8] = {w[0], 0u, w[2], 0u, 0u, 0u, 0u, w[7]};
        if (strspu_is_audio(h, j.rules)) {
            audio = true;
            const int64_t k = strspu_chunk_number(h);
            psxhip_str_sector_t e = {PSXHIP_STR_SECTOR_AUDIO, -1, -1, (int32_t)(strspu_chunk_flags(h) & 1u)};
            if (k >= 0 && k < (int64_t)j.audio_capacity) {
                const size_t at = (size_t)s * j.audio_capacity + (size_t)k;
                atomicMin(j.d_owner + at, (uint32_t)i);
                atomicAdd(j.d_count + at, 1u);
                e.index = (int32_t)k;
            } else {
                dropped = true;
            }
            if (j.d_user_table) j.d_user_table[(size_t)s * j.n_sectors + i] = e;
        }
    }
    const unsigned long long m_audio = __ballot(audio), m_dropped = __ballot(dropped);
    if (lane == 0 && m_audio) {
        psxhip_str_summary_t* sum = j.d_summary + s;
        const int n = (int)__popcll(m_audio);
        atomicAdd(&sum->n_audio, n);
        atomicSub(&sum->n_other, n);
        if (m_dropped) atomicAdd(&sum->n_dropped_audio, (int)__popcll(m_dropped));
    }
}

template <bool kVec16>
__global__ __launch_bounds__(256) void spu_deinterleave_kernel(const psxhip_spu_deinterleave_job_t j) {
    const int s = (int)blockIdx.y;
    const uint32_t per = (uint32_t)(j.channels * j.blocks);                    // records per chunk
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;                        // the record: (k B + b) channels + c = k per + r
    if (g >= (uint32_t)j.n_chunks * per) return;
    const uint32_t k = g / per, r = g - k * per;
    const uint32_t b = r / (uint32_t)j.channels, c = r - b * (uint32_t)j.channels;
    int32_t src = (int32_t)k;
    if (j.src_chunk) src = j.src_chunk[(size_t)s * j.src_stream_stride + k];
    if (src < 0) return;
    const uint8_t* p = j.in + (size_t)s * j.in_stream_stride + (size_t)src * j.chunk_stride + j.lane_offset +
                       ((size_t)c * (size_t)j.blocks + b) * 16u;
    uint4 v;
    if (kVec16) {
        v = *(const uint4*)p;
    } else {
        const uint32_t* w = (const uint32_t*)p;
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    *(uint4*)(j.units + (size_t)s * j.units_stream_stride + (size_t)g * 16u) = v;
}

__global__ __launch_bounds__(256) void strspu_demux_finish_kernel(const psxhip_strspu_demux_job_t j) {
    const int tid = (int)threadIdx.x, lane = tid & 63, s = (int)blockIdx.y;
    const int k = (int)blockIdx.x * 256 + tid;
    bool owned = false, last = false;
    if (k < j.audio_capacity) {
        const size_t at = (size_t)s * j.audio_capacity + (size_t)k;
        const uint32_t own = j.d_owner[at];
        psxhip_strspu_chunk_info_t info = {-1, PSXHIP_STRSPU_CHUNK_MISSING, 0, 0, 0, 0, 0, 0};
        if (own < (uint32_t)j.n_sectors) {
            owned = true;
            const uint32_t* w = sector_words(j, s, own);
            const uint32_t h[8] = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
            const uint32_t flags = strspu_chunk_flags(h);
            int32_t st = 0;
            if (j.d_count[at] > 1u) st |= PSXHIP_STRSPU_CHUNK_DUPLICATE;
            if (strspu_chunk_mismatch(h, (int64_t)k, j.rules)) st |= PSXHIP_STRSPU_CHUNK_MISMATCH;
            info.first_sector = (int32_t)own;
            info.status = st;
            info.channels = (int32_t)(h[4] & 0xFFFFu);
            info.lane_bytes = (int32_t)(h[4] >> 16);
            info.frequency = (int32_t)h[5];
            info.first_sample = (int32_t)h[6];
            info.flags = (int32_t)flags;
            last = (flags & 1u) != 0u;
        }
        j.d_chunk_info[at] = info;
    }
    const unsigned long long m_owned = __ballot(owned), m_last = __ballot(last);
    if (lane == 0 && m_owned) {
        psxhip_strspu_audio_summary_t* a = j.d_audio_summary + s;
        const int base = k;                                                    // (lane 0's number)
        atomicAdd(&a->n_complete, (int)__popcll(m_owned));
        atomicMax(&a->n_chunks, base + 64 - (int)__clzll((long long)m_owned));
        if (m_last) atomicMin((uint32_t*)&a->last_chunk, (uint32_t)(base + __ffsll((long long)m_last) - 1));
    }
}

}  // namespace

extern "C" int psxhip_spu_deinterleave_launch(const psxhip_spu_deinterleave_job_t* j, int n_streams, void* stream) {
    const size_t total = (size_t)j->n_chunks * (size_t)j->channels * (size_t)j->blocks;
    if (!total) return PSXHIP_OK;
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)n_streams);
    if (j->vec16)
        hipLaunchKernelGGL(spu_deinterleave_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *j);
    else
        hipLaunchKernelGGL(spu_deinterleave_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *j);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}

extern "C" int psxhip_strspu_demux_launch(int device, const psxhip_strspu_demux_job_t* j, void* stream) {
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    hipStream_t st = (hipStream_t)stream;
    const size_t S = (size_t)j->n_streams, words = S * (size_t)j->audio_capacity;
    if (words) {
        HIP_TRY(hipMemsetAsync(j->d_owner, 0xFF, words * sizeof(uint32_t), st), PSXHIP_EDEVICE);
        HIP_TRY(hipMemsetAsync(j->d_count, 0, words * sizeof(uint32_t), st), PSXHIP_EDEVICE);
    }
    hipLaunchKernelGGL(strspu_demux_init_kernel, dim3((unsigned)((j->n_streams + 255) / 256)), dim3(256), 0, st, *j);
    if (j->n_sectors > 0 && j->rules.ch != 0)
        hipLaunchKernelGGL(strspu_demux_scan_kernel, dim3((unsigned)((j->n_sectors + 255) / 256), (unsigned)j->n_streams), dim3(256), 0, st, *j);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    if (j->audio_capacity > 0) {
        if (j->n_sectors > 0 && j->rules.ch != 0) {
            psxhip_spu_deinterleave_job_t d;
            d.in = j->d_sectors;
            d.in_stream_stride = j->in_stream_stride;
            d.chunk_stride = kSector;
            d.lane_offset = 0x20;
            d.blocks = 126 / j->rules.ch;
            d.channels = j->rules.ch;
            d.n_chunks = j->audio_capacity;
            d.src_chunk = (const int32_t*)j->d_owner;                          // all ones = -1: no owner, the chunk is skipped
            d.src_stream_stride = (size_t)j->audio_capacity;
            d.units = j->d_units;
            d.units_stream_stride = j->units_stream_stride;
            d.vec16 = ((uintptr_t)j->d_sectors & 15) == 0 && (j->n_streams == 1 || (j->in_stream_stride & 15) == 0);
            rc = psxhip_spu_deinterleave_launch(&d, j->n_streams, stream);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(strspu_demux_finish_kernel, dim3((unsigned)((j->audio_capacity + 255) / 256), (unsigned)j->n_streams), dim3(256), 0,
                           st, *j);
        HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    }
    return PSXHIP_OK;
}
