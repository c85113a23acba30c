"""jampack_amd -- MI355X (gfx950) implementation of Jampack's block hot path behind the reference's own
bwt.hpp / ans.hpp / rank.hpp interface.  The compute path is libjampack_amd.so (hand-written HIP kernels);
importing this package loads it and fails loudly if it has not been built."""
from . import corpus  # noqa: F401
from ._lib import ABI_SYMBOLS, CHUNK, LIB_PATH, TRAILER, JampackError, lib  # noqa: F401
from .api import (blocks_compress_multi, blocks_decompress_multi, multi_plan, Ans, Bwt, Checksum, Context, Postcoder, ans_capacity, block_compress, block_decompress,  # noqa: F401
                  jam_block_read, jam_block_write, jam_compress, jam_compress_bound, jam_decompress, jam_frames, jam_index, jam_cli_index, jam_read, JamIndex, Lz77, Lpx, Filters, checksum_host,
                  jam_cli_block_read, jam_cli_block_write, jam_cli_compress, jam_cli_compress_bound, cli_stages_bound, cli_stages_encode, CLI_DEDUPE, CLI_FILTERS, filters_cost, jam_cli_decompress, jam_cli_decompress_all, jam_cli_frames, JAM_STAGED, jam_staged_block_read, jam_staged_block_write,
                  jam_staged_compress, jam_staged_compress_bound, jam_staged_decompress, jam_staged_frames, jam_staged_index, lz77_size, lz77_deep_limits, JAM_INDEX_PLAIN, JAM_INDEX_CLI, JAM_INDEX_STAGED, JAM_GAP_NOFRAME, JAM_GAP_STAGE, jam_recover_index, jam_salvage, jam_repair, jam_update, jam_update_bound, init, shutdown, release_idle, thread_device, ans_decoded_size)

lib()  # no lazy fallback: the HIP extension must be present
