"""GPU: every `_host` variant with a `_batch` twin gives the bytes its twin gives.  Three items of seeded random input go through
`_host` on numpy buffers and through `_batch` on device tensors the test makes itself (the reference: the library's staging never
touches them); every output must be byte-identical.  Three items is the smallest count at which a wrong stride or a swapped buffer
shows.  Functions with optional pointers run with all of them given and with all of them left out, and once with only the optional
outputs left out: the required outputs must not change then."""
import numpy as np
import pytest

import ddn

pytestmark = pytest.mark.gpu

N = 3
U8, I8, I16, U16, I32, U32, I64, U64, F32 = "u1", "i1", "i2", "u2", "i4", "u4", "i8", "u8", "f4"


def A(role, dtype, count, lo=0, hi=2):
    """a pointer argument: role in / out / io (both), o-prefixed when optional; inputs are integers of [lo, hi) (floats: that scale),
    or the array given for `lo` (carried state that holds indices starts as the library initialises it)"""
    return (role, dtype, count, lo, hi)


BATCH_ONLY_NULL = ("batch-only",)   # a pointer only the batched call has, left null
S16_STATE = np.tile(np.r_[25.0, np.zeros(31)], N)   # ddn_audio_s16_state_init
GAIN = np.array([25.0, 10.0, 40.0])                  # state->aout_gain of three talk paths
PUNCT = np.array([1, 1, 0, 1], np.uint8)   # a host array in both calls

# one line per function: the arguments of the `_host` call in order (the twin takes the same and a stream)
CALLS = {
    "ddn_fec_p25_12_soft_host": [A("in", I16, N * 196, -3000, 3000), N, A("out", U8, N * 12), A("oout", I32, N)],
    "ddn_fec_r34_host": [A("in", U8, N * 98, 0, 4), A("oin", U8, N * 98, 0, 256), N, A("out", U8, N * 18)],
    "ddn_fec_nxdn_conv_host": [A("in", U8, N * 2 * 20, 0, 3), A("oin", U8, N * 2 * 20, 0, 256), N, 20, 16, A("oio", U16, N * 16, 0, 1000),
                               A("out", U8, N * 2), 2],
    "ddn_fec_viterbi_k5_host": [A("in", U16, N * 42, 0, 65536), N, 42, PUNCT, 4, A("out", U8, N * 8), 8, A("oout", U32, N)],
    "ddn_p25p1_nid_decode_host": [A("in", U8, N * 63), A("oin", U8, N * 63, 0, 256), A("oin", I32, N, 0, 4096), A("oin", U8, N),
                                  A("oin", U8, N, 0, 256), 64, N, A("out", I32, N * 4)],
    "ddn_p25p1_imbe_deinterleave_host": [A("in", U8, 400 * 10, 0, 256), 400, A("in", I64, N, 0, 300), A("in", I32, N, 0, 36), N,
                                         A("out", U8, N * 184), A("out", U8, N * 368), A("out", U8, N), A("out", I32, N)],
    "ddn_fec_p25_crc16_host": [A("in", U8, N * 12, 0, 256), 12, N, A("out", U8, N)],
    "ddn_fec_p25_lsd_host": [A("io", U8, N * 16), A("oin", I16, N * 16, -3000, 3000), N, A("out", U8, N)],
    "ddn_fec_hamming_10_6_3_host": [A("io", U8, N * 10), N, A("out", U8, N)],
    "ddn_fec_golay24_host": [12, A("io", U8, N * 12), A("in", U8, N * 12), N, A("out", U8, N), A("oout", I32, N)],
    "ddn_fec_p25_rs_host": [1, A("io", U8, N * 16 * 6), A("in", U8, N * 8 * 6), N, A("out", U8, N)],
    "ddn_fec_rs28_host": [0, A("io", U8, N * 96), A("in", U8, N * 168), A("oin", I8, N * 28, 0, 44), A("oin", U8, N, 0, 5), N, A("out", I32, N)],
    "ddn_audio_s16_host": [A("in", F32, N * 2 * 160, 0, 3000), N, 2, 0.0, 1, 1, A("out", I16, N * 2 * 160), A("io", F32, N * 32, S16_STATE),
                           A("io", F32, N, GAIN)],
    "ddn_fec_bptc_128x77_host": [A("in", U8, N * 128), N, A("out", U8, N * 77), A("oout", U32, N)],
    "ddn_fec_bptc_16x2_host": [A("in", U8, N * 32), N, 1, A("out", U8, N * 32), A("oout", U32, N)],
    "ddn_fec_isch_lookup_host": [A("in", U64, N, 0, 1 << 40), A("oin", U8, N * 40, 0, 256), N, A("out", I32, N)],
    "ddn_fec_golay24_soft_host": [6, A("io", U8, N * 6), A("in", U8, N * 12), A("in", I32, N * 18, 0, 256), N, A("out", U8, N),
                                  A("oout", I32, N)],
    "ddn_fec_hamming_10_6_3_soft_host": [A("in", U8, N * 10), A("in", I32, N * 10, 0, 256), N, A("out", U8, N * 10), A("out", U8, N)],
    "ddn_fec_p25_rs_soft_host": [2, A("io", U8, N * 20 * 6), A("in", U8, N * 16 * 6), A("in", U8, N * 20, 0, 256), A("in", U8, N * 16, 0, 256), N,
                                 A("out", U8, N)],
    "ddn_fec_p25_12_soft_list_host": [A("in", I16, N * 196, -3000, 3000), N, 8, A("out", U8, N * 8 * 16), A("out", I32, N)],
    "ddn_fec_r34_list_host": [A("in", U8, N * 98, 0, 4), A("oin", U8, N * 98, 0, 256), N, 32, A("out", U8, N * 32 * 24), A("out", I32, N)],
    "ddn_fec_block_code_host": [1, A("io", U8, N * 12 * 2), N, 2, A("oout", U8, N * 8 * 2), A("oout", U8, N)],
    "ddn_fec_bptc_196x96_host": [A("in", U8, N * 196), 1, N, A("out", U8, N * 96), A("oout", U8, N * 3), A("oout", U32, N)],
    "ddn_fec_trellis_decode_host": [A("in", U8, N * 22), 22, N, 8, A("out", U8, N * 8), 8],
    "ddn_fec_rs_12_9_host": [A("io", U8, N * 12, 0, 256), N, A("out", U8, N), A("oout", U8, N), A("oout", U8, N * 3)],
    "ddn_audio_agf_host": [A("io", F32, N * 2 * 160, 0, 3000), N, 2, 0.0, 0, A("io", F32, N, GAIN)],
    "ddn_fec_p25_mbf34_list_host": [A("in", I16, N * 196, -3000, 3000), N, 8, BATCH_ONLY_NULL, A("out", U8, N * 8 * 24), A("out", I32, N)],
    "ddn_p25p2_mac_crc_host": [1, A("in", U8, N * 180), N, A("out", U8, N), A("oout", U8, N)],
    "ddn_p25p2_ess_host": [A("in", U8, N * 96), A("in", I16, N * 96, -3000, 3000), A("in", U8, N * 168), A("in", I16, N * 168, -3000, 3000), N, 0,
                           A("out", U8, N * 96), A("out", I32, N), A("out", U8, N)],
    "ddn_p25p2_groups_host": [A("in", U8, N * 1400), A("in", I16, N * 1400, -3000, 3000), N, 1, A("oin", I32, N, 0, 2), A("in", U64, N, 1, 1 << 44),
                              A("io", U8, N * 592, 0, 1), 0, A("io", I32, N * 4 * 8, 0, 1), A("io", U8, N * 4 * 180, 0, 1),
                              A("io", U8, N * 4 * 384, 0, 1), A("io", U8, N * 4 * 384, 0, 1), A("io", U8, N * 4 * 96, 0, 1)],
    "ddn_p25p2_sync_cut_host": [A("in", U8, N * 1500, 0, 4), A("in", I16, N * 1500 * 2, -3000, 3000), N, 1500, 1500, A("oin", I32, N, 0, 1), 1,
                                A("out", I32, N), A("io", I32, N, 0, 1), A("out", I32, N), A("io", U8, N * 1400, 0, 1), A("io", I16, N * 1400, 0, 1)],
    "ddn_p25p2_burst_fields_host": [A("in", U8, N * 360), A("in", I16, N * 360, -3000, 3000), N, 0, A("out", I32, N), A("out", I32, N)],
    "ddn_p25p2_xcch_host": [1, A("in", U8, N * 360), A("in", I16, N * 360, -3000, 3000), N, 0, A("out", U8, N * 180), A("out", I32, N),
                            A("out", U8, N)],
}


def test_every_host_variant_with_a_batched_twin_is_compared():
    twins = sorted(k for k in ddn.PROTOTYPES if k.endswith("_host") and k[:-5] + "_batch" in ddn.PROTOTYPES)
    assert sorted(CALLS) == twins


def _base(role):
    return role[1:] if role in ("oin", "oout", "oio") else role


def _is_ptr(a):
    return isinstance(a, tuple) and a is not BATCH_ONLY_NULL


def _run(name, seed, omit):
    """both paths on the same random input; `omit`: the roles left null.  -> {argument index: (host bytes, batch bytes)} of the outputs"""
    import torch
    rng = np.random.default_rng(seed)
    l = ddn.lib()
    h_args, b_args, outs, alive = [], [], {}, []     # alive: every buffer stays until both calls are through
    for k, a in enumerate(CALLS[name]):
        if a is BATCH_ONLY_NULL:
            b_args.append(None)
            continue
        if isinstance(a, np.ndarray):
            h_args.append(a.ctypes.data)
            b_args.append(a.ctypes.data)
            continue
        if not _is_ptr(a):
            h_args.append(a)
            b_args.append(a)
            continue
        role, dtype, count, lo, hi = a
        # (drawn also where the argument is then left out: the other inputs stay the same between the runs)
        if isinstance(lo, np.ndarray):
            v = lo.astype(dtype)
        else:
            v = (rng.normal(0, hi, count) if dtype == F32 else rng.integers(lo, hi, count)).astype(dtype)
        if _base(role) == "out":
            v = np.zeros(count, dtype)
        if role in omit:
            h_args.append(None)
            b_args.append(None)
            continue
        d = torch.from_numpy(v.copy()).cuda()
        alive += [v, d]
        h_args.append(v.ctypes.data)
        b_args.append(d.data_ptr())
        if _base(role) in ("out", "io"):
            outs[k] = (role, v, d)
    assert getattr(l, name)(*h_args) == 0, l.ddn_last_error()
    assert getattr(l, name[:-5] + "_batch")(*b_args, None) == 0, l.ddn_last_error()
    torch.cuda.synchronize()
    return {k: (role, v.tobytes(), d.cpu().numpy().tobytes()) for k, (role, v, d) in outs.items()}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_host_variant_gives_its_batched_twin_s_bytes(built, name):
    seed = sorted(CALLS).index(name)
    full = _run(name, seed, omit=())
    assert full and all(h == b for _, h, b in full.values()), [k for k, (_, h, b) in full.items() if h != b]
    roles = {a[0] for a in CALLS[name] if _is_ptr(a)}
    if not any(r.startswith("o") for r in roles):
        return
    bare = _run(name, seed, omit=("oin", "oout", "oio"))
    assert all(h == b for _, h, b in bare.values()), [k for k, (_, h, b) in bare.items() if h != b]
    if "oout" in roles:  # only the optional outputs left out: the required ones do not change
        fewer = _run(name, seed, omit=("oout",))
        for k, (role, h, b) in fewer.items():
            assert h == b and h == full[k][1], k
