"""psxavenc_amd -- MI355X-native implementation of psxavenc's MDEC BS encode path and SPU/XA ADPCM
search, behind the reference's own function surfaces (see DESIGN.md / INTEGRATION.md).

The product is ``libpsxav_hip.so`` (C ABI, include/*.h).  This package is the thin Python mirror used
by tests and bench.py: device memory and streams come from PyTorch, everything else from the library.
"""
from ._lib import LIB_PATH, PsxHipError, lib  # noqa: F401

BS_CODEC_V2, BS_CODEC_V3, BS_CODEC_V3DC = 0, 1, 2   # bs_codec_t, psxavenc/args.h:61-65

from .decode import MdecDecoder, psnr  # noqa: E402,F401
from . import display  # noqa: E402,F401  (display.kernel_rev(): the revision of the display back-end's kernels)
from .display import DISPLAY_CHROMA_BILINEAR, DISPLAY_DITHER, DISPLAY_MASK_BIT, OUT_RGB24, OUT_RGB555, OUT_RGBX32  # noqa: E402,F401
from . import ingest  # noqa: E402,F401  (ingest.kernel_rev(): the revision of the picture ingest's kernels)
from .ingest import Ingest, ingest_scale_device  # noqa: E402,F401
from . import adpcm_decode  # noqa: E402,F401  (adpcm_decode.kernel_rev(): the revision of the ADPCM decoder's kernels)
from .adpcm_decode import (adpcm_sse, decode_chains_chunked, decode_chains_device, snr_db, spu_decode_streams,  # noqa: E402,F401
                           xa_decode_streams, xa_disassemble)
from . import strdemux  # noqa: E402,F401  (strdemux.kernel_rev(): the revision of the STR reader's kernels)
from .strdemux import StrReader, spu_deinterleave_device  # noqa: E402,F401
from . import disc  # noqa: E402,F401  (disc.kernel_rev(): the revision of the disc finisher's kernels)
from .disc import disc_check, disc_finish, disc_plan  # noqa: E402,F401
from . import discread  # noqa: E402,F401  (discread.kernel_rev(): the revision of the disc reader's kernels)
from .discread import DiscReader, disc_read, disc_read_host  # noqa: E402,F401
from . import spubank  # noqa: E402,F401  (spubank.kernel_rev(): the revision of the sound bank's kernels)
from .spubank import SpuBank  # noqa: E402,F401
