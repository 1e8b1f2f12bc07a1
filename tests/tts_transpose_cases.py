"""Inputs of the tile-stream transposed product and value gradient (tests/test_gpu_tts_transpose.py, test_gpu_tts_value_grad.py,
test_tts_transpose_host.py), in one place.  No product code; not a test module and not a conftest.

| case                     | what it reaches                                                                              | width |
| tile_stream  (AUTO)      | 3 tiles, one block each of 24 chunks, rows cut by chunk boundaries                           | 1     |
| tts_cut_row  (AUTO)      | a quarter of the rows empty (fillers), one row in pieces: 2 carry tiles + `fix`              | 1     |
| xlds_A       (TTS)       | 13 tiles, 3 carry tiles, 57 entries in the fullest column                                    | 4     |
| two_blocks_3000  (TTS)   | two blocks per tile (the 48-slice limit: 5 M columns cut every slice short)                  | 2     |
| two_blocks_20000 (TTS)   | two blocks per tile, 7 292 fillers (rows absent from a block), tiles of up to 6 792 rows     | 1     |
| small_band (TTS_SMALL)   | the 13 K-slot geometry (transposed only: it cannot be updatable)                             | 4     |
width: step_small_cases.tts_widths(tts, cols)[1], the vectors a pass of linear_device_t / value_grad_device takes."""
import step_small_cases as S


def two_blocks_3000():
    return S.uniform(3000, 5_000_000, 72000, 404, dict(format=1, group=28), name="two_blocks_3000")


def two_blocks_20000():
    return S.uniform(20000, 5_000_000, 72000, 407, dict(format=1, group=28), name="two_blocks_20000")


# name -> (matrix, environment, geometry of prep_from_coo(..., tts=(0, geometry)), pass width)
CASES = {
    "tile_stream": (S.tile_stream, S.AUTO, 0, 1),
    "tts_cut_row": (S.tile_stream_cut_row, S.AUTO, 0, 1),
    "xlds_A": (lambda: S.xlds_cases()["A"], S.TTS, 0, 4),
    "two_blocks_3000": (two_blocks_3000, S.TTS, 0, 2),
    "two_blocks_20000": (two_blocks_20000, S.TTS, 0, 1),
    "small_band": (S.small_band, S.TTS_SMALL, 1, 4),
}
UPDATABLE = list(CASES)[:5]


def case(name):
    make, env, geometry, width = CASES[name]
    return make(), env, geometry, width
