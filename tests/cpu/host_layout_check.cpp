// host_layout_check.cpp -- prints what psxavenc_amd/csrc/host_layout.h derives, one line per case with the case's own parameters in
// front, for tests/test_host_layout_cpu.py to compare with numbers it works out itself.  Built with the host sanitizers: the tables
// are exactly as long as the fillers are told, so a write past them is reported.
#include <stdio.h>

#include <vector>

#include "../../psxavenc_amd/csrc/host_layout.h"

static void print_chains(const std::vector<psxhip_adpcm_chain_t>& chains, const std::vector<int32_t>& base) {
    for (size_t i = 0; i < chains.size(); i++)
        printf(" | %lld %d %d %d %d %d", (long long)chains[i].sample_offset, chains[i].pitch, chains[i].sample_limit, chains[i].n_units,
               chains[i].unit_stride, base[i]);
    printf("\n");
}

int main() {
    for (int format = 0; format < 2; format++)
        for (int bits = 4; bits <= 8; bits += 4)
            for (int stereo = 0; stereo < 2; stereo++) {
                const XaLayout x = xa_layout(format, stereo, bits);
                printf("xa %d %d %d : %d %d %d %d %d %d\n", format, stereo, bits, x.channels, x.units_per_group, x.units_per_sector, x.sector_bytes,
                       x.samples_per_sector, x.record_bytes);
                printf("xa_interleave %d %d %d : %d %d\n", format, stereo, bits, xa_sector_interleave(stereo, 18900, bits), xa_sector_interleave(stereo, 37800, bits));
            }
    for (int format : {6, 7, 9, 8}) {
        int size = -7, sub = -7, hdr = -7;                      // an unknown format leaves them alone
        const bool ok = str_sector_geometry(format, &size, &sub, &hdr);
        printf("geo %d : %d %d %d %d\n", format, (int)ok, size, sub, hdr);
    }
    for (int n_streams : {1, 3})
        for (int pitch : {1, 2}) {
            const int n_units = 5, limit = 28 * n_units - 3;
            const long long stride = (long long)limit * pitch + 11;          // larger than a stream
            std::vector<psxhip_adpcm_chain_t> chains((size_t)n_streams);
            std::vector<int32_t> base((size_t)n_streams);
            fill_planar_chains(chains.data(), base.data(), n_streams, stride, pitch, limit, n_units);
            printf("planar %d %lld %d %d %d", n_streams, stride, pitch, limit, n_units);
            print_chains(chains, base);
        }
    for (int n_streams : {1, 3})
        for (int channels : {1, 2}) {
            const int units_per_stream = 144, limit = 28 * units_per_stream / channels - 9;
            const long long stride = (long long)limit * channels + 13;       // larger than a stream
            std::vector<psxhip_adpcm_chain_t> chains((size_t)n_streams * channels);
            std::vector<int32_t> base((size_t)n_streams * channels);
            fill_interleaved_chains(chains.data(), base.data(), n_streams, channels, stride, limit, units_per_stream);
            printf("interleaved %d %d %lld %d %d", n_streams, channels, stride, limit, units_per_stream);
            print_chains(chains, base);
        }
    // the per-call path's fixed tables of four: entries past n_chains stay as they were
    {
        psxhip_adpcm_chain_t chains[4] = {};
        int32_t base[4] = {-1, -1, -1, -1};
        fill_interleaved_chains(chains, base, 1, 2, 0, 100, 144);
        printf("fixed4 : %d %d %d %d | %d %d\n", base[0], base[1], base[2], base[3], chains[2].n_units, chains[3].pitch);
    }
    BumpOffsets o;
    printf("bump :");
    for (size_t bytes : {(size_t)0, (size_t)1, (size_t)256, (size_t)257}) printf(" %zu", o.take(bytes));
    printf(" %zu\n", o.end);
    return 0;
}
