"""The grid caps of the launchers in echoseal_amd/csrc/*.hip, and where the suite drives each of them past its cap.

Most launchers size their grid with es_grid(items, per_block, cap_blocks): past `per_block * cap_blocks` items the blocks take a second
trip round their grid-stride loop.  `trip(device)` restates those products (the formulas are the launchers' own), `past(cap)` is the
launch size the tests use, `index_set` the rows a host or oracle check looks at, and LAUNCHERS says for every capped launcher which
test takes it past its cap, or why none can in seconds.  tests/test_grid_caps_listed.py holds the table to the sources.

A plain helper module: no fixtures, nothing pytest collects."""
from collections import namedtuple

import numpy as np

XC_WAVES = 4                    # csrc/es_internal.h: waves per block of the correlation kernels (float64, float32 screen, stream)
PW_WAVES = 4                    # csrc/es_sync32.hip: rows per block of es_pick_exact_wave_kernel
MEMO_BLOCK = 256                # csrc/es_memo.hip: records per workgroup (its grid is not capped)


def trip(device=None) -> dict:
    """Items one trip of each capped launch covers on `device`: what es_grid caps the grid at, times the items of a block."""
    import torch
    cu = torch.cuda.get_device_properties(device if device is not None else 0).multi_processor_count
    return {
        "cu": cu,
        "tx_symbols": 16 * cu,              # es_tx_symbols_kernel, es_tx_symbols_keyed_kernel: a frame per block, 16 * cu blocks
        "tx_finish": 64 * cu,               # es_tx_finish_kernel: four frames (waves) per block, 16 * cu blocks
        "polar_encode": 32 * cu,            # es_polar_encode_kernel: four frames per block, 8 * cu blocks
        "lane": 8 * cu * 256,               # one lane per record, 8 * cu blocks of 256: AEAD, select, schedule, key ring, hop window
        "mix_block": 2048 * cu,             # es_mix_*_block_kernel: an audio block per workgroup, 2048 * cu workgroups
        "pick_rows": 16 * cu,               # es_pick_kernel, es_pick_ragged_kernel, es_pick_at_kernel: a row per block, 16 * cu blocks
        "xcorr_blocks": 16 * cu,            # es_xcorr_kernel and its ragged / stream / float32 forms: 16 * cu blocks of XC_WAVES waves ...
        "xcorr_segments": 16 * cu * XC_WAVES,   # ... a wave per (row, segment of 1216 lags)
        "pick_exact_rows": 16 * cu * PW_WAVES,  # es_pick_exact_wave_kernel: a row per wave, 16 * cu blocks of PW_WAVES waves
    }


def past(cap: int) -> int:
    """A launch size above `cap` with a margin, and no multiple of any block size (cap is a multiple of 16; the precedent is
    cap + 4099 in test_gpu_aead_edges.py)."""
    return cap + cap // 16 + 5


def index_set(n: int, trips, seed: int = 0) -> np.ndarray:
    """The rows of an n-row launch a host or oracle check looks at: k*t - 1, k*t, k*t + 1 for every trip boundary k*t < n of every
    trip size t in `trips`, row 0, the last row and 16 seeded random rows.  Sorted, unique."""
    rows = {0, n - 1}
    for t in np.atleast_1d(trips).tolist():
        for edge in range(t, n, t):
            rows |= {edge - 1, edge, edge + 1}
    rows |= set(np.random.default_rng(seed).integers(0, n, 16).tolist())
    return np.array(sorted(r for r in rows if 0 <= r < n), np.int64)


def slices(n: int, step: int):
    """Consecutive slices of at most `step` rows that cover n rows."""
    return [slice(lo, min(n, lo + step)) for lo in range(0, n, step)]


Driven = namedtuple("Driven", "file test note", defaults=("",))      # the test that launches past the cap and compares with a reference
Exempt = namedtuple("Exempt", "why")                                 # one sentence: why no test can do that in seconds

_A = "test_gpu_grid_stride.py"
_B = "test_gpu_grid_stride_dsp.py"
_WAVE_MIX = ("only the workgroup-per-block kernel: the one-wave-per-block kernel of block = 1024 strides past 4 * 2048 * num_cu blocks "
             "of 1 024 samples, about 8.6 GB of samples per operand")

LAUNCHERS = {
    # es_aead.hip
    "es_launch_aead_check": Driven("test_gpu_aead_edges.py", "test_grid_stride_check_and_seal"),
    "es_launch_aead_seal": Driven("test_gpu_aead_edges.py", "test_grid_stride_check_and_seal"),
    "es_launch_select": Driven("test_gpu_aead_edges.py", "test_select_grid_stride"),
    "es_launch_aead_check_keyed": Driven(_A, "test_keyed_aead_past_the_cap"),
    "es_launch_select_keyed": Driven(_A, "test_keyed_aead_past_the_cap"),
    "es_launch_aead_seal_keyed": Driven(_A, "test_keyed_aead_past_the_cap"),
    # es_keyring.hip
    "es_launch_keyring_derive": Driven(_A, "test_key_ring_past_the_cap"),
    "es_launch_schedule_keyed": Driven(_A, "test_keyed_schedule_past_the_cap"),
    "es_launch_hop_window": Driven(_A, "test_hop_window_past_the_cap"),
    # es_llr.hip
    "es_launch_llr": Driven("test_gpu_front_edges.py", "test_llr_device_filling_large_build",
                            "four times num_cu * 64 records, each against the oracle; variant 0 of the small build at 65 536 records in "
                            "test_gpu_headline_oracle.py::test_headline_step_every_record_vs_oracle"),
    "es_launch_header": Driven("test_gpu_front_edges.py", "test_header_device_filling"),
    # es_mix.hip
    "es_launch_mix": Driven(_B, "test_mix_block_kernel_past_the_cap", _WAVE_MIX),
    "es_launch_mix_ragged": Driven(_B, "test_ragged_mix_block_kernel_past_the_cap", _WAVE_MIX),
    "es_launch_mix_stream": Driven(_B, "test_stream_mix_block_kernel_past_the_cap", _WAVE_MIX),
    "es_launch_stream_commit": Exempt("A workgroup per chunk under a cap of 2048 * num_cu: a second trip needs more than half a million "
                                      "live streams in one tick, each with a table row of 1 215 chips."),
    # es_resample.hip
    "es_launch_resample": Driven("test_gpu_resample_arms.py", "test_resample_grid_stride_wraps"),
    "es_launch_resample_ragged": Exempt("Its cap is 2^31 - 1 blocks, a tile each: no batch that fits the device reaches it."),
    "es_launch_resample_stream": Exempt("Its cap is 2^31 - 1 blocks, a tile each: no tick that fits the device reaches it."),
    # es_sched.hip
    "es_launch_schedule": Driven("test_gpu_parity.py", "test_schedule_kernel_vs_oracle", "2^20 counters, 64 seeded rows against the host schedule"),
    # es_scl.hip, es_scl_wide.hip
    "es_launch_softplus": Driven("test_gpu_parity.py", "test_device_softplus_bits", "over three million arguments, each against the oracle"),
    "es_launch_polar_encode": Driven(_A, "test_polar_encode_past_the_cap"),
    "es_launch_polar_f_dev": Driven("test_softplus_dev_gpu.py", "test_device_polar_f_dev_bits", "over 2.5 million pairs, each against the host C form"),
    # es_sync.hip
    "es_launch_xcorr": Driven(_B, "test_float64_sync_past_the_cap"),
    "es_launch_pick": Driven(_B, "test_float64_sync_past_the_cap"),
    "es_launch_xcorr_ragged": Driven(_B, "test_ragged_sync_past_the_cap"),
    "es_launch_pick_ragged": Driven(_B, "test_ragged_sync_past_the_cap"),
    "es_launch_xcorr_stream": Driven(_B, "test_live_monitor_many_streams"),
    "es_launch_pick_at": Driven(_B, "test_live_monitor_many_streams"),
    # es_sync32.hip
    "es_launch_xcorr32": Driven(_B, "test_two_kernel_sync_past_the_cap"),
    "es_launch_pick_exact": Driven(_B, "test_two_kernel_sync_past_the_cap"),
    "es_launch_sync_fused": Driven("test_gpu_sync_screen.py", "test_capacity_of_a_launch"),
    # es_tx.hip
    "es_launch_tx_frames": Driven(_A, "test_frame_generator_past_the_cap"),
    "es_launch_tx_frames_keyed": Driven(_A, "test_keyed_frame_generator_past_the_cap"),
}
