// sector_kernels.hip -- CD-ROM XA sectors on the device for MI355X (gfx950), hand-written HIP: ADPCM unit records into XA sound
// sectors with their EDC (adpcm.c:193-233,266-332; cdrom.c:28-41,55-74,102-110) and back, and the video sectors of a muxed STR
// stream (filefmt.c:462-475, mdec.c:782-832).  One 256-thread workgroup per sector; the EDC is one wavefront's work (xa_edc.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psxhip_adpcm_internal.h"
#include "xa_edc.h"

namespace {

// the unit records of the ADPCM kernels (adpcm_kernels.hip): 32 bytes with 8-bit codes, an SPU block of 16 with 4-bit codes
constexpr int kRecordBytes = 32;
constexpr int kRecordBytes4 = 16;

__device__ __forceinline__ uint8_t to_bcd(int v) { return (uint8_t)(v + (v / 10) * 6); }

// ---- XA sector assembly.  One 256-thread workgroup per sector; the sector is built in LDS as a full
// 2352-byte raw sector (the .xa form simply skips the first 16 bytes on write-out, adpcm.c:303-311).
__global__ __launch_bounds__(256) void xa_assemble_kernel(const psxhip_xa_job_t job) {
    __shared__ __attribute__((aligned(16))) uint8_t sec[2352];
    __shared__ uint32_t crc_tab[256];
    const int tid = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const bool four = job.bits == 4;
    const int upg = four ? 8 : 4;                 // sound units per group
    const int sector_size = job.format == 0 ? 2336 : 2352;
    uint32_t* const sec32 = (uint32_t*)sec;

    crc_tab[tid] = c_xa_tables[tid];
    for (int i = tid; i < 2352 / 4; i += 256) sec32[i] = 0u;
    __syncthreads();

    if (tid == 255) {
        if (job.format == 1) {       // psx_cdrom_init_sector, mode 2 (cdrom.c:55-74)
            for (int i = 1; i <= 10; i++) sec[i] = 0xFF;
            const int lba = job.first_lba + (job.dst_sector ? job.dst_sector[s] : s) + 150;
            sec[12] = to_bcd(lba / 4500);
            sec[13] = to_bcd((lba / 75) % 60);
            sec[14] = to_bcd(lba % 75);
            sec[15] = 0x02;
        }
        sec[16] = (uint8_t)job.file_number;
        sec[17] = (uint8_t)(job.channel_number & 0x1F);
        sec[18] = (uint8_t)(0x04 | 0x20 | 0x40);   // AUDIO | FORM2 | RT
        sec[19] = (uint8_t)((job.stereo ? 0x01 : 0) | (job.frequency == 37800 ? 0 : 0x04) | (four ? 0 : 0x10));
        sec[20] = sec[16]; sec[21] = sec[17]; sec[22] = sec[18]; sec[23] = sec[19];
    }

    // sound groups: 18 x 128 bytes at sector offset 0x18 (adpcm.c:193-233,311-322)
    const uint8_t* rec0 = job.units + (size_t)blockIdx.y * job.units_stream_stride + (size_t)s * 18 * upg * (four ? kRecordBytes4 : kRecordBytes);
    if (four) {
        // 4-bit: sample w of the group's 8 units is the 4 bytes (u0 | u1 << 4, u2 | u3 << 4, u4 | u5 << 4, u6 | u7 << 4) at group
        // byte 16 + 4 w.  A record is an SPU block: [header][0][14 code bytes, two samples each].  Thread (group, q) reads dword q
        // of the 8 records -- code bytes 4 q - 2 .. 4 q + 1, i.e. samples 8 q - 4 .. 8 q + 3 (q = 0: its upper half only) -- pairs
        // the low nibbles (even samples) and the high nibbles (odd samples) of unit pairs for four code bytes at once, and
        // transposes 4 x 4 bytes twice: 32 contiguous sector bytes from 8 dword loads.
        if (tid < 18 * 4) {
            const int g = tid >> 2, q = tid & 3;
            const uint32_t* gr = (const uint32_t*)(rec0 + (size_t)g * 8 * kRecordBytes4) + q;
            uint32_t pe[4], po[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t lo = gr[(2 * c) * (kRecordBytes4 / 4)], hi = gr[(2 * c + 1) * (kRecordBytes4 / 4)];
                pe[c] = (lo & 0x0F0F0F0Fu) | ((hi << 4) & 0xF0F0F0F0u);          // byte j: column c of the EVEN sample of code byte j
                po[c] = ((lo >> 4) & 0x0F0F0F0Fu) | (hi & 0xF0F0F0F0u);          // ... of the ODD sample
            }
            // transpose: e[j] = (pe0.j, pe1.j, pe2.j, pe3.j) = the four bytes of sample 2 * (code byte j), o[j] likewise of the sample after it
            uint32_t e[4], o[4];
            {
                const uint32_t a0 = __builtin_amdgcn_perm(pe[1], pe[0], 0x05010400u), a1 = __builtin_amdgcn_perm(pe[1], pe[0], 0x07030602u);
                const uint32_t b0 = __builtin_amdgcn_perm(pe[3], pe[2], 0x05010400u), b1 = __builtin_amdgcn_perm(pe[3], pe[2], 0x07030602u);
                e[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u); e[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
                e[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u); e[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
            }
            {
                const uint32_t a0 = __builtin_amdgcn_perm(po[1], po[0], 0x05010400u), a1 = __builtin_amdgcn_perm(po[1], po[0], 0x07030602u);
                const uint32_t b0 = __builtin_amdgcn_perm(po[3], po[2], 0x05010400u), b1 = __builtin_amdgcn_perm(po[3], po[2], 0x07030602u);
                o[0] = __builtin_amdgcn_perm(b0, a0, 0x05040100u); o[1] = __builtin_amdgcn_perm(b0, a0, 0x07060302u);
                o[2] = __builtin_amdgcn_perm(b1, a1, 0x05040100u); o[3] = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
            }
            // dword q holds record bytes 4 q .. 4 q + 3 = code bytes 4 q - 2 + j: samples 2 (4 q - 2 + j) and the one after
            uint32_t* grp = sec32 + (0x18 + g * 128 + 16) / 4;        // the group's 28 sample dwords
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int cb = 4 * q - 2 + j;                         // code byte (q = 0: j = 0, 1 are header and flags)
                if (cb >= 0) { grp[2 * cb] = e[j]; grp[2 * cb + 1] = o[j]; }
            }
        } else if (tid >= 128 && tid < 128 + 18 * 2) {
            // header bytes: units {0,1,2,3} at 0..3 and 4..7, units {4..7} at 8..11 and 12..15
            const int g = (tid - 128) >> 1, half = (tid - 128) & 1;
            const uint8_t* gr = rec0 + (size_t)g * 8 * kRecordBytes4 + (size_t)half * 4 * kRecordBytes4;
            const uint32_t h = (uint32_t)gr[0] | (uint32_t)gr[kRecordBytes4] << 8 | (uint32_t)gr[2 * kRecordBytes4] << 16 | (uint32_t)gr[3 * kRecordBytes4] << 24;
            uint32_t* dst = sec32 + (0x18 + g * 128 + 8 * half) / 4;
            dst[0] = h; dst[1] = h;
        }
    } else {
        for (int i = tid; i < 18 * 128; i += 256) {
            const int g = i >> 7, b = i & 127;
            const uint8_t* gr = rec0 + (size_t)g * upg * kRecordBytes;
            uint8_t v;
            if (b < 16) {
                // 8-bit: units 0..3 at 0..3 and 4..7, bytes 8..15 are never written by the reference (stay 0)
                v = b < 8 ? gr[(b & 3) * kRecordBytes] : 0;
            } else {
                const int w = (b - 16) >> 2, col = (b - 16) & 3;          // sample index, byte column
                v = gr[col * kRecordBytes + 4 + w];
            }
            sec[0x18 + i] = v;
        }
    }
    __syncthreads();

    // form-2 EDC over sector bytes 0x10 .. 0x92B (2332 bytes) -> 0x92C (cdrom.c:102-110): one wavefront (edc_wave).
    // (Before round 4: 256 chunks of 10 bytes, every thread advancing its partial to the END of the span through up to eight
    // bit-matrix products out of LDS -- four wavefronts x 8 products of 32 conditional xors where one wavefront x 6 does.)
    if (tid < 64) {
        const uint32_t c = edc_wave<kEdcSpan>(sec32, crc_tab, tid);
        if (tid == 0) sec32[0x92C / 4] = c;
        // psx_audio_xa_encode_finalize (adpcm.c:334-340) ORs EOF into both subheader copies AFTER the EDC was
        // computed and does not refresh it; kept that way for byte parity.  (Same wavefront, behind its reads of the span.)
        if (tid == 1 && (job.eof_flags ? job.eof_flags[s] != 0 : (s < 32 && ((job.eof_bits >> s) & 1u)))) {
            sec[18] |= 0x80;
            sec[22] = sec[18];
        }
    }
    __syncthreads();

    const int lead = 2352 - sector_size;
    uint8_t* dst = job.out + (size_t)blockIdx.y * job.out_stream_stride + (size_t)(job.dst_sector ? job.dst_sector[s] : s) * sector_size;
    for (int i = tid; i < sector_size / 4; i += 256) ((uint32_t*)dst)[i] = *(const uint32_t*)&sec[lead + 4 * i];
}

// ---- STR video sectors (psxhip_str_encode_device): what encode_file_str does around encode_sector_str for every video slot of the
// stream (filefmt.c:462-475 with :73-91, mdec.c:782-832, cdrom.c:92-100) -- sector header and subheaders, the 32-byte chunk header,
// 2016 bytes of the frame's bitstream, the form-1 EDC -- one workgroup per sector, the frames' bitstreams and results read where the
// frame kernel left them in HBM.  tab[i] = {slot n in the stream, frame (-2: an audio slot with no samples left: a zero sector),
// byte offset into the frame's bitstream, the frame's budget}.
__global__ __launch_bounds__(256) void str_video_sector_kernel(const psxhip_str_video_job_t job) {
    __shared__ __attribute__((aligned(16))) uint8_t sec[2352];
    __shared__ uint32_t crc_tab[256];
    const int tid = (int)threadIdx.x;
    uint32_t* const sec32 = (uint32_t*)sec;
    const int4 e = job.tab[blockIdx.x];
    const int n = e.x, frame = e.y, offset = e.z, budget = e.w;
    uint8_t* dst = job.out + (size_t)blockIdx.y * job.out_stream_stride + (size_t)n * (size_t)job.sector_size;
    if (frame < 0) {        // an audio slot with no samples left: psx_audio_xa_encode writes nothing (adpcm.c:310); zero here
        for (int i = tid; i < job.sector_size / 4; i += 256) ((uint32_t*)dst)[i] = 0u;
        return;
    }
    crc_tab[tid] = c_xa_tables[tid];
    for (int i = tid; i < 2352 / 4; i += 256) sec32[i] = 0u;
    __syncthreads();
    const int at = job.format == 6 ? 0x08 : (job.format == 7 ? 0x18 : 0x00);          // mdec.c:822-829
    const uint8_t* fo = job.bs + (size_t)blockIdx.y * job.bs_stream_stride + (size_t)frame * job.bs_stride;
    // the 2016 payload bytes: 504 dwords (the frame's bitstream and its slices are dword-aligned, and so is at + 0x20)
    for (int i = tid; i < 2016 / 4; i += 256) sec32[(at + 0x20) / 4 + i] = ((const uint32_t*)(fo + offset))[i];
    if (tid == 255) {
        uint8_t* sub = nullptr;
        if (job.format == 7) {               // psx_cdrom_init_sector(.., MODE2_FORM1), cdrom.c:55-74
            for (int i = 1; i <= 10; i++) sec[i] = 0xFF;
            const int lba = n + 150;
            sec[12] = to_bcd(lba / 4500);
            sec[13] = to_bcd((lba / 75) % 60);
            sec[14] = to_bcd(lba % 75);
            sec[15] = 0x02;
            sub = sec + 16;
        } else if (job.format == 6) {
            sub = sec;
        }
        if (sub) {                           // init_sector_buffer_video, filefmt.c:73-91
            sub[0] = (uint8_t)job.xa_file;
            sub[1] = (uint8_t)(job.xa_channel & 0x1F);
            sub[2] = (uint8_t)(0x08 | 0x40);     // DATA | RT
            sub[3] = 0;
            sub[4] = sub[0]; sub[5] = sub[1]; sub[6] = sub[2]; sub[7] = sub[3];
        }
        // the chunk header of encode_sector_str, mdec.c:782-820
        uint8_t* hd = sec + at;
        const unsigned bytes_used = (unsigned)job.res[(size_t)blockIdx.y * job.frames_per_stream + frame].bytes_used;
        const unsigned fi = (unsigned)(frame + 1);          // frame_index counts from 1
        hd[0x00] = 0x60; hd[0x01] = 0x01;
        hd[0x02] = (uint8_t)job.video_id; hd[0x03] = (uint8_t)(job.video_id >> 8);
        hd[0x04] = (uint8_t)(offset / 2016); hd[0x05] = (uint8_t)((offset / 2016) >> 8);
        hd[0x06] = (uint8_t)(budget / 2016); hd[0x07] = (uint8_t)((budget / 2016) >> 8);
        hd[0x08] = (uint8_t)fi; hd[0x09] = (uint8_t)(fi >> 8); hd[0x0A] = (uint8_t)(fi >> 16); hd[0x0B] = (uint8_t)(fi >> 24);
        hd[0x0C] = (uint8_t)bytes_used; hd[0x0D] = (uint8_t)(bytes_used >> 8); hd[0x0E] = (uint8_t)(bytes_used >> 16); hd[0x0F] = (uint8_t)(bytes_used >> 24);
        hd[0x10] = (uint8_t)job.width; hd[0x11] = (uint8_t)(job.width >> 8);
        hd[0x12] = (uint8_t)job.height; hd[0x13] = (uint8_t)(job.height >> 8);
        for (int i = 0; i < 8; i++) hd[0x14 + i] = fo[i];       // the BS header of the frame
        hd[0x1C] = 0; hd[0x1D] = 0; hd[0x1E] = 0; hd[0x1F] = 0;
    }
    __syncthreads();
    // psx_cdrom_calculate_checksums(.., MODE2_FORM1) as the reference's muxer calls it for every flavour (filefmt.c:474): the EDC of
    // buffer bytes 0x10 .. 0x817 at 0x818 (the ECC behind it is not computed, cdrom.c:99)
    if (tid < 64) {
        const uint32_t c = edc_wave<kEdcSpanForm1>(sec32, crc_tab, tid);
        if (tid == 0) sec32[0x818 / 4] = c;
    }
    __syncthreads();
    for (int i = tid; i < job.sector_size / 4; i += 256) ((uint32_t*)dst)[i] = sec32[i];
}

// ---- XA sectors -> unit records in encode order: the inverse of xa_assemble_kernel, one workgroup per sector
__global__ __launch_bounds__(256) void xa_disassemble_kernel(const psxhip_xa_dis_job_t job) {
    __shared__ __attribute__((aligned(16))) uint8_t sec[2352];
    __shared__ uint32_t crc_tab[256];
    __shared__ int status;
    const int tid = (int)threadIdx.x;
    const int s = (int)blockIdx.x;
    const bool four = job.bits == 4;
    const int sector_size = job.format == 0 ? 2336 : 2352;
    const int lead = 2352 - sector_size;
    uint32_t* const sec32 = (uint32_t*)sec;

    crc_tab[tid] = c_xa_tables[tid];
    if (tid == 0) status = 0;
    if (tid < lead / 4) sec32[tid] = 0u;
    const uint32_t* src = (const uint32_t*)(job.sectors + (size_t)s * sector_size);
    for (int i = tid; i < sector_size / 4; i += 256) sec32[lead / 4 + i] = src[i];
    __syncthreads();

    int bad = 0;
    if (tid < 18) {
        // a sound group's header copies: bytes 4..7 against 0..3, 12..15 against 8..11 (adpcm.c:212-219)
        const uint32_t* grp = sec32 + (0x18 + tid * 128) / 4;
        if (grp[0] != grp[1] || grp[2] != grp[3]) bad |= 1;
    }
    if (tid >= 64 && tid < 128) {
        // one wavefront: subheaders, coding byte, the form-2 EDC over sector bytes 0x10 .. 0x92B (cdrom.c:102-110)
        const int l = tid - 64;
        const uint32_t sub0 = sec32[4], sub1 = sec32[5], stored = sec32[0x92C / 4];
        if (l == 0) {
            if (sub0 != sub1) bad |= 2;
            const uint32_t coding = (uint32_t)((job.stereo ? 0x01 : 0) | (job.frequency == 37800 ? 0 : 0x04) | (four ? 0 : 0x10));
            if ((sub0 >> 24) != coding) bad |= 4;
        }
        // psx_audio_xa_encode_finalize sets EOF in both subheaders behind the EDC and leaves the EDC as it was (adpcm.c:334-340):
        // such a sector carries the EDC of the sector without the bits.  The CRC is linear over GF(2): that is this sector's EDC xor
        // the EDC of a span that holds the two bits alone -- a constant (eof_edc_delta, from the host)
        const uint32_t edc = (uint32_t)__shfl((int)edc_wave<kEdcSpan>(sec32, crc_tab, l), 0, 64);
        const bool eof = (sub0 & sub1 & 0x00800000u) != 0u;
        const bool ok = stored == 0u || stored == edc || (eof && stored == (edc ^ job.eof_edc_delta));
        if (l == 0 && !ok) bad |= 8;
    }
    if (bad) atomicOr(&status, bad);

    // 18 sound groups of 128 bytes at sector byte 0x18; 576 record dwords per sector either way
    uint32_t* dst = (uint32_t*)job.units + (size_t)s * 576;
    for (int i = tid; i < 576; i += 256) {
        uint32_t v = 0;
        if (four) {
            // unit n of group g: header at group byte n (n < 4) or n + 4; sample w is nibble n & 1 of group byte 16 + 4 w + n / 2.  The
            // record is an SPU block: [header][0][14 code bytes: sample 2 k low, 2 k + 1 high]
            const int ui = i >> 2, q = i & 3, g = ui >> 3, n = ui & 7;
            const uint8_t* grp = sec + 0x18 + g * 128;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int rb = 4 * q + k;
                uint32_t byte = 0;
                if (rb == 0) byte = grp[n + (n >= 4 ? 4 : 0)];
                else if (rb >= 2) {
                    const int w = 2 * (rb - 2), sh = 4 * (n & 1);
                    byte = ((grp[16 + 4 * w + (n >> 1)] >> sh) & 15u) | (((grp[16 + 4 * (w + 1) + (n >> 1)] >> sh) & 15u) << 4);
                }
                v |= byte << (8 * k);
            }
        } else {
            // unit n of group g: header at group byte n; sample w at group byte 16 + 4 w + n.  Record: [header][0][0][0][28 codes]
            const int ui = i >> 3, q = i & 7, g = ui >> 2, n = ui & 3;
            const uint8_t* grp = sec + 0x18 + g * 128;
            if (q == 0) v = grp[n];
            else {
#pragma unroll
                for (int k = 0; k < 4; k++) v |= (uint32_t)grp[16 + 4 * (4 * (q - 1) + k) + n] << (8 * k);
            }
        }
        dst[i] = v;
    }
    __syncthreads();
    if (tid == 0 && job.status) job.status[s] = status;
}
}  // namespace

extern "C" int psxhip_sector_tables(int device) { return xa_tables(device); }

extern "C" hipError_t psxhip_xa_assemble_launch(const psxhip_xa_job_t* j, int n_streams, void* stream) {
    hipLaunchKernelGGL(xa_assemble_kernel, dim3((unsigned)j->n_sectors, (unsigned)n_streams), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_str_video_sectors_launch(const psxhip_str_video_job_t* j, int n_streams, void* stream) {
    hipLaunchKernelGGL(str_video_sector_kernel, dim3((unsigned)j->n_entries, (unsigned)n_streams), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}

extern "C" hipError_t psxhip_xa_disassemble_launch(const psxhip_xa_dis_job_t* j, void* stream) {
    hipLaunchKernelGGL(xa_disassemble_kernel, dim3((unsigned)j->n_sectors), dim3(256), 0, (hipStream_t)stream, *j);
    return hipGetLastError();
}
