// str_demux_kernels.hip -- the STR / STRCD / STRV reader's kernels (psxhip_str_demux_device; include/psxav_hip.h):
// muxed sectors -> one row per frame for the BS decoder, the XA sectors compacted in stream order, a record per frame, a table entry
// per sector.  The inverse of str_video_sector_kernel (adpcm_kernels.hip) and of the sector schedule; the rules are "psxhip STR demux
// v1", restated sequentially in tests/str_demux_ref.py.  Five launches, nothing read back:
//   scan    one thread per sector reads the subheader and the first 12 bytes of the chunk header, classifies the sector, ranks the
//           audio sectors inside its block of 256, takes the stream's smallest frame_index and the counts by kind
//   prefix  one workgroup per stream turns the blocks' audio counts into exclusive prefix sums
//   place   one thread per sector: audio ordinal = block prefix + rank; video row = frame_index - first_frame, the lowest position per
//           (row, chunk) and the lead per row by integer atomicMin on words of their own
//   gather  one workgroup per sector: audio sectors are copied to their ordinal; a row's video sector is staged in LDS, its payload
//           stored to the row when it owns its (row, chunk), its header compared with the lead's, its EDC checked by one wavefront per span
//   finish  one thread per row: info, status, size, the count of whole frames
// Every index that comes from the stream's bytes -- row, chunk, ordinal, lead -- is compared with its bound before it addresses memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_internal.h"
#include "psxhip_str_demux_internal.h"
#include "xa_edc.h"

namespace {

constexpr int kChunk = 2016;                    // payload bytes of a video sector (mdec.c:832)
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kBlock = PSXHIP_STR_DEMUX_SCAN_BLOCK;
static_assert(kBlock == 256, "the scan, prefix and place passes are written for four wavefronts");

// what the scan pass keeps of a sector: x = kind | EOF << 8, y = frame_index, z = chunk_index | chunk_count << 16, w = audio rank in the block
__device__ __forceinline__ const uint32_t* sector_words(const psxhip_str_demux_job_t& j, int s, uint32_t pos) {
    return (const uint32_t*)(j.d_sectors + (size_t)s * j.in_stream_stride + (size_t)pos * (size_t)j.sector_size);
}

// the first_frame in effect: the caller's, or the smallest frame_index of the stream's video sectors (0 without one)
__device__ __forceinline__ int64_t first_frame_of(const psxhip_str_demux_job_t& j, int s) {
    if (j.first_frame >= 0) return j.first_frame;
    const uint32_t mn = j.d_min[s];
    return mn == kNone ? 0 : (int64_t)mn;
}

__global__ __launch_bounds__(256) void str_demux_scan_kernel(const psxhip_str_demux_job_t j) {
    __shared__ uint32_t w_audio[4], w_video[4], w_min[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, s = (int)blockIdx.y;
    const int i = (int)blockIdx.x * kBlock + tid;
    uint32_t kind = PSXHIP_STR_SECTOR_EMPTY, eof = 0, fi = kNone, chunk = 0;
    const bool in = i < j.n_sectors;
    if (in) {
        const uint32_t* w = sector_words(j, s, (uint32_t)i);
        uint32_t sub = 0;
        bool audio = false;
        if (j.sub_at >= 0) {
            sub = w[j.sub_at >> 2];
            const int file = (int)(sub & 0xFF), channel = (int)((sub >> 8) & 0x1F);
            audio = j.audio_on && (sub & 0x040000u) && (j.xa_file == -1 || file == j.xa_file) &&
                    (j.xa_channel == -1 || channel == (j.xa_channel & 0x1F));
        }
        const uint32_t h0 = w[j.hdr_at >> 2];
        if (audio) {
            kind = PSXHIP_STR_SECTOR_AUDIO;
            eof = (sub >> 23) & 1u;
        } else if (!(sub & 0x040000u) && (h0 & 0xFFFFu) == 0x0160u && (j.video_id == -1 || (int)(h0 >> 16) == j.video_id)) {
            kind = PSXHIP_STR_SECTOR_VIDEO;
            chunk = w[(j.hdr_at >> 2) + 1];
            fi = w[(j.hdr_at >> 2) + 2];
        }
    }
    const bool is_audio = kind == PSXHIP_STR_SECTOR_AUDIO, is_video = kind == PSXHIP_STR_SECTOR_VIDEO;
    const unsigned long long m_audio = __ballot(is_audio), m_video = __ballot(is_video);
    uint32_t mn = is_video ? fi : kNone;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)mn, d, 64);
        mn = o < mn ? o : mn;
    }
    if (lane == 0) {
        w_audio[wv] = (uint32_t)__popcll(m_audio);
        w_video[wv] = (uint32_t)__popcll(m_video);
        w_min[wv] = mn;
    }
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(m_audio & ((1ull << lane) - 1ull));
    for (int k = 0; k < wv; k++) rank += w_audio[k];
    if (in) {
        uint4 rec;
        rec.x = kind | eof << 8;
        rec.y = fi;
        rec.z = chunk;
        rec.w = rank;
        ((uint4*)j.d_rec)[(size_t)s * j.n_sectors + i] = rec;
    }
    if (tid == 0) {
        const uint32_t na = w_audio[0] + w_audio[1] + w_audio[2] + w_audio[3], nv = w_video[0] + w_video[1] + w_video[2] + w_video[3];
        const int here = j.n_sectors - (int)blockIdx.x * kBlock;
        const uint32_t valid = (uint32_t)(here < kBlock ? here : kBlock);
        j.d_blocks[(size_t)s * j.n_blocks + blockIdx.x] = na;
        psxhip_str_summary_t* sum = j.d_summary + s;
        if (nv) atomicAdd(&sum->n_video, (int)nv);
        if (na) atomicAdd(&sum->n_audio, (int)na);
        if (valid - nv - na) atomicAdd(&sum->n_other, (int)(valid - nv - na));
        uint32_t m = w_min[0];
        for (int k = 1; k < 4; k++) m = w_min[k] < m ? w_min[k] : m;
        if (m != kNone) atomicMin(j.d_min + s, m);
    }
}

__global__ __launch_bounds__(256) void str_demux_prefix_kernel(const psxhip_str_demux_job_t j) {
    __shared__ uint32_t w_sum[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, s = (int)blockIdx.x;
    uint32_t* const b = j.d_blocks + (size_t)s * j.n_blocks;
    uint32_t carry = 0;
    for (int base = 0; base < j.n_blocks; base += kBlock) {
        const int idx = base + tid;
        const uint32_t v = idx < j.n_blocks ? b[idx] : 0u;
        uint32_t x = v;                                            // inclusive sum over the wavefront
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)x, d, 64);
            if (lane >= d) x += t;
        }
        if (lane == 63) w_sum[wv] = x;
        __syncthreads();
        uint32_t before = 0;
        for (int k = 0; k < wv; k++) before += w_sum[k];
        if (idx < j.n_blocks) b[idx] = carry + before + x - v;
        carry += w_sum[0] + w_sum[1] + w_sum[2] + w_sum[3];
        __syncthreads();
    }
    if (tid == 0) j.d_summary[s].first_frame = j.d_min[s] == kNone ? 0u : (uint32_t)first_frame_of(j, s);
}

__global__ __launch_bounds__(256) void str_demux_place_kernel(const psxhip_str_demux_job_t j) {
    __shared__ uint32_t drop_video, drop_audio, rows;
    const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
    const int i = (int)blockIdx.x * kBlock + tid;
    if (tid == 0) { drop_video = 0; drop_audio = 0; rows = 0; }
    __syncthreads();
    if (i < j.n_sectors) {
        const uint4 rec = ((const uint4*)j.d_rec)[(size_t)s * j.n_sectors + i];
        psxhip_str_sector_t e;
        e.kind = (int32_t)(rec.x & 0xFF);
        e.frame = -1;
        e.index = -1;
        e.eof = 0;
        if (e.kind == PSXHIP_STR_SECTOR_AUDIO) {
            const uint32_t k = j.d_blocks[(size_t)s * j.n_blocks + blockIdx.x] + rec.w;
            e.index = (int32_t)k;
            e.eof = (int32_t)((rec.x >> 8) & 1u);
            if (k >= (uint32_t)j.xa_capacity) atomicAdd(&drop_audio, 1u);
        } else if (e.kind == PSXHIP_STR_SECTOR_VIDEO) {
            const uint32_t cidx = rec.z & 0xFFFFu, ccnt = rec.z >> 16;
            const int64_t row = (int64_t)rec.y - first_frame_of(j, s);
            e.index = (int32_t)cidx;
            if (row >= 0 && row < (int64_t)j.max_frames) {
                e.frame = (int32_t)row;
                const size_t r = (size_t)s * j.max_frames + (size_t)row;
                if (cidx < ccnt && cidx < (uint32_t)j.chunk_cap) {
                    atomicMin(j.d_owner + r * (size_t)j.chunk_cap + cidx, (uint32_t)i);
                } else {
                    e.eof = PSXHIP_STR_FRAME_RANGE;
                    atomicOr(j.d_status + r, (uint32_t)PSXHIP_STR_FRAME_RANGE);
                }
                atomicMin(j.d_lead + r, (cidx ? 0x80000000u : 0u) | (uint32_t)i);
                atomicMax(&rows, (uint32_t)row + 1u);
            } else {
                atomicAdd(&drop_video, 1u);
            }
        }
        j.d_table[(size_t)s * j.n_sectors + i] = e;
    }
    __syncthreads();
    if (tid == 0) {
        psxhip_str_summary_t* sum = j.d_summary + s;
        if (drop_video) atomicAdd(&sum->n_dropped_video, (int)drop_video);
        if (drop_audio) atomicAdd(&sum->n_dropped_audio, (int)drop_audio);
        if (rows) atomicMax(&sum->n_rows, (int)rows);
    }
}

__global__ __launch_bounds__(256) void str_demux_gather_kernel(const psxhip_str_demux_job_t j) {
    // four dwords of room in front of the sector: the EDC of sector bytes 0 .. 0x807 is edc_wave on a base 16 bytes down
    __shared__ __attribute__((aligned(16))) uint32_t buf[4 + 2352 / 4];
    __shared__ uint32_t crc_tab[256], edc[2];
    const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
    const uint32_t i = blockIdx.x;
    const size_t at = (size_t)s * j.n_sectors + i;
    psxhip_str_sector_t e = j.d_table[at];
    const uint32_t* const src = sector_words(j, s, i);
    const int words = j.sector_size / 4;
    if (e.kind != PSXHIP_STR_SECTOR_VIDEO || e.frame < 0 || e.frame >= j.max_frames) {
        if (e.kind == PSXHIP_STR_SECTOR_AUDIO && e.index >= 0 && e.index < j.xa_capacity) {
            uint32_t* dst = (uint32_t*)(j.d_xa + (size_t)s * j.xa_stream_stride + (size_t)e.index * (size_t)j.sector_size);
            for (int k = tid; k < words; k += 256) dst[k] = src[k];
        }
        if (j.d_user_table && tid == 0) j.d_user_table[at] = e;
        return;
    }
    uint32_t* const sec32 = buf + 4;
    for (int k = tid; k < words; k += 256) sec32[k] = src[k];
    if (tid < 4) buf[tid] = 0u;
    crc_tab[tid] = c_xa_tables[tid];
    __syncthreads();

    const size_t r = (size_t)s * j.max_frames + (size_t)e.frame;
    const uint32_t cidx = (uint32_t)e.index;
    const uint32_t* const h = sec32 + (j.hdr_at >> 2);
    const bool placeable = !(e.eof & PSXHIP_STR_FRAME_RANGE) && cidx < (uint32_t)j.chunk_cap;
    const bool placed = placeable && j.d_owner[r * (size_t)j.chunk_cap + cidx] == i;
    if (placed) {
        uint32_t* dst = (uint32_t*)(j.d_bs + (size_t)s * j.bs_stream_stride + (size_t)e.frame * j.bs_stride + (size_t)cidx * kChunk);
        for (int k = tid; k < kChunk / 4; k += 256) dst[k] = h[8 + k];
    }

    // ---- the EDC rule.  STRCD: the EDC of bytes 0x10 .. 0x817 at 0x818, a zero word is not checked.  STR: that (the muxer's placement),
    // or the EDC of bytes 0 .. 0x807 at 0x808 (a disc's), or both words zero.  One wavefront per span, side by side.
    if (tid < 128 && j.format != 9 && (tid < 64 || j.format == 6)) {
        const uint32_t c = edc_wave<kEdcSpanForm1>(tid < 64 ? sec32 : buf, crc_tab, tid & 63);
        if ((tid & 63) == 0) edc[tid >> 6] = c;
    }
    __syncthreads();
    if (tid != 0) return;
    bool bad = false;
    if (j.format == 7) {
        bad = sec32[0x818 / 4] != 0u && sec32[0x818 / 4] != edc[0];
    } else if (j.format == 6) {
        const uint32_t as_muxed = sec32[0x818 / 4], on_disc = sec32[0x808 / 4];
        bad = as_muxed != edc[0] && on_disc != edc[1] && (as_muxed | on_disc) != 0u;
    }
    // ---- the comparison with the lead, the row's status bits
    uint32_t lead = j.d_lead[r] & 0x7FFFFFFFu;
    if (lead >= (uint32_t)j.n_sectors) lead = i;
    const uint32_t* const lh = sector_words(j, s, lead) + (j.hdr_at >> 2);
    bool mismatch = (h[1] >> 16) != (lh[1] >> 16) || h[3] != lh[3] || h[4] != lh[4] || h[5] != lh[5] || h[6] != lh[6];
    if (lead == i && cidx == 0) mismatch = mismatch || h[5] != h[8] || h[6] != h[9];
    uint32_t bits = 0;
    if (bad) bits |= PSXHIP_STR_FRAME_EDC;
    if (mismatch) bits |= PSXHIP_STR_FRAME_MISMATCH;
    if (placeable && !placed) bits |= PSXHIP_STR_FRAME_DUPLICATE;
    if (bits) atomicOr(j.d_status + r, bits);
    if (j.d_user_table) {
        if (bad) e.eof |= PSXHIP_STR_FRAME_EDC;
        j.d_user_table[at] = e;
    }
}

__global__ __launch_bounds__(256) void str_demux_finish_kernel(const psxhip_str_demux_job_t j) {
    const int tid = (int)threadIdx.x, s = (int)blockIdx.y;
    const int row = (int)blockIdx.x * 256 + tid;
    bool whole = false;
    if (row < j.max_frames) {
        const size_t r = (size_t)s * j.max_frames + (size_t)row;
        psxhip_str_frame_info_t info = {0u, 0, 0, 0u, 0, 0, 0, PSXHIP_STR_FRAME_MISSING};
        int32_t size = 0;
        const uint32_t lk = j.d_lead[r], lead = lk & 0x7FFFFFFFu;
        if (lk != kNone && lead < (uint32_t)j.n_sectors) {
            const uint32_t* const lh = sector_words(j, s, lead) + (j.hdr_at >> 2);
            const uint32_t ccnt = lh[1] >> 16;
            info.frame_index = lh[2];
            info.chunk_count = (int32_t)ccnt;
            info.bytes_used = lh[3];
            info.width = (int32_t)(lh[4] & 0xFFFFu);
            info.height = (int32_t)(lh[4] >> 16);
            info.first_sector = (int32_t)lead;
            bool missing = ccnt == 0u || ccnt > (uint32_t)j.chunk_cap;
            int placed = 0;
            const uint32_t* own = j.d_owner + r * (size_t)j.chunk_cap;
            for (int c = 0; c < j.chunk_cap; c++) {
                const bool has = own[c] != kNone;
                placed += has;
                if ((uint32_t)c < ccnt && !has) missing = true;
            }
            info.chunks_placed = placed;
            uint32_t st = j.d_status[r];
            if (missing) st |= PSXHIP_STR_FRAME_MISSING;
            if ((j.width && j.width != info.width) || (j.height && j.height != info.height)) st |= PSXHIP_STR_FRAME_GEOMETRY;
            info.status = (int32_t)st;
            size = missing ? 0 : (int32_t)ccnt * kChunk;
            whole = !missing;
        }
        j.d_info[r] = info;
        j.d_bs_sizes[r] = size;
    }
    const unsigned long long m = __ballot(whole);
    if ((tid & 63) == 0 && m) atomicAdd(&j.d_summary[s].n_complete, (int)__popcll(m));
}

}  // namespace

extern "C" int psxhip_str_demux_launch(int device, const psxhip_str_demux_job_t* j, void* stream) {
    int rc = psxhip_ensure_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device), PSXHIP_EDEVICE);
    rc = xa_tables(device);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t S = (size_t)j->n_streams, rows = S * (size_t)j->max_frames;
    // d_owner, d_lead and d_min lie back to back (psxhip_str_demux.cpp lays the workspace out so): one fill with ones
    HIP_TRY(hipMemsetAsync(j->d_owner, 0xFF, (rows * (size_t)j->chunk_cap + rows + S) * sizeof(uint32_t), st), PSXHIP_EDEVICE);
    if (rows) HIP_TRY(hipMemsetAsync(j->d_status, 0, rows * sizeof(uint32_t), st), PSXHIP_EDEVICE);
    HIP_TRY(hipMemsetAsync(j->d_summary, 0, S * sizeof(psxhip_str_summary_t), st), PSXHIP_EDEVICE);
    if (j->n_sectors > 0) {
        const dim3 per_sector((unsigned)j->n_blocks, (unsigned)j->n_streams);
        hipLaunchKernelGGL(str_demux_scan_kernel, per_sector, dim3(256), 0, st, *j);
        hipLaunchKernelGGL(str_demux_prefix_kernel, dim3((unsigned)j->n_streams), dim3(256), 0, st, *j);
        hipLaunchKernelGGL(str_demux_place_kernel, per_sector, dim3(256), 0, st, *j);
        hipLaunchKernelGGL(str_demux_gather_kernel, dim3((unsigned)j->n_sectors, (unsigned)j->n_streams), dim3(256), 0, st, *j);
    }
    if (j->max_frames > 0)
        hipLaunchKernelGGL(str_demux_finish_kernel, dim3((unsigned)((j->max_frames + 255) / 256), (unsigned)j->n_streams), dim3(256), 0, st, *j);
    HIP_TRY(hipGetLastError(), PSXHIP_EDEVICE);
    return PSXHIP_OK;
}
