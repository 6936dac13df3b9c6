"""CPU-only checks of the sampling test helpers (tests/sampling_cases.py) and of the host side of lhrs_sample_rows: Philox known answers, the
float64 reference against the installed transformers' processors, a comparator that rejects every planted mistake, and the C-ABI / Python
surface of the device sampler (rejections happen on the host, before any launch)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_cases as SC  # noqa: E402

SEED = 0x1234_5678_9ABC_DEF0


# ------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    assert " ".join(f"{w:08x}" for w in SC.philox4x32_10(ctr, key)) == want


def test_bitmap_round_trip():
    seen = SC.make_seen(2, 1000, 3)
    for r in range(2):
        assert (SC.bitmap_to_bool(SC.bool_to_bitmap(seen[r]), 1000) == seen[r]).all()


# ------------------------------------------------------------------------------------------------ reference vs HF
@pytest.mark.parametrize("V", SC.VOCABS)
@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("params", SC.GRID, ids=lambda p: f"t{p.temperature}-k{p.top_k}-p{p.top_p}-r{p.penalty}")
def test_reference_support_matches_hf(params, scale, V):
    logits = SC.make_logits(3, V, scale, seed=11).numpy()
    seen = SC.make_seen(3, V, seed=12)
    for r in range(3):
        ref = SC.ref_sample64(logits[r], seen[r], params)
        hf = SC.hf_support(logits[r], np.nonzero(seen[r])[0], params)
        assert (hf == ref.support).all(), (r, np.nonzero(hf != ref.support)[0])
        assert ref.support[np.argmax(ref.z)] and abs(ref.probs.sum() - 1) < 1e-12


# ------------------------------------------------------------------------------------------------ comparator
def _case(params, V=32000, scale=1, row=0):
    return SC.make_logits(2, V, scale, seed=21).numpy()[row], SC.make_seen(2, V, seed=22)[row]


@pytest.mark.parametrize("V", (32000, 1000))
@pytest.mark.parametrize("scale", SC.SCALES)
@pytest.mark.parametrize("params", SC.GRID, ids=lambda p: f"t{p.temperature}-k{p.top_k}-p{p.top_p}-r{p.penalty}")
def test_comparator_accepts_reference_in_kernel_formats(params, scale, V):
    logits, seen = _case(params, V, scale)
    ref = SC.ref_sample64(logits, seen, params)
    w = SC.emulate_weights(logits, seen, params)
    assert w.max() == SC.WEIGHT_ONE
    for step in range(4):
        m = SC.check(w, ref, SC.draw_from_weights(w, SEED, step, 1), SEED, step, 1, "emulated")
        assert m.n_excused == 0


def _rejects(w, ref, **kw):
    with pytest.raises(AssertionError):
        SC.check(w, ref, **kw)


def test_comparator_rejects_missing_penalty():
    p = SC.Params(1.0, 50, 0.95, 1.05)
    for scale in SC.SCALES:
        logits, seen = _case(p, scale=scale)
        seen = seen.copy()
        seen[np.argsort(-logits)[:20:2]] = True   # the penalty matters where tokens that can be drawn have been seen
        _rejects(SC.emulate_weights(logits, seen, p._replace(penalty=1.0)), SC.ref_sample64(logits, seen, p))


@pytest.mark.parametrize("params", SC.GRID, ids=lambda p: f"t{p.temperature}-k{p.top_k}-p{p.top_p}-r{p.penalty}")
def test_comparator_rejects_temperature_off_by_5_percent(params):
    logits, seen = _case(params)
    _rejects(SC.emulate_weights(logits, seen, params._replace(temperature=params.temperature * 1.05)), SC.ref_sample64(logits, seen, params))


def test_comparator_rejects_top_k_off_by_one():
    for p in (SC.Params(0.7, 5, 1.0, 1.0), SC.Params(0.4, 50, 1.0, 1.0)):
        logits, seen = _case(p)
        ref = SC.ref_sample64(logits, seen, p)
        for k in (p.top_k - 1, p.top_k + 1):
            _rejects(SC.emulate_weights(logits, seen, p._replace(top_k=k)), ref)


def test_comparator_rejects_top_p_cut_one_token_early_and_late():
    p = SC.Params(0.4, 50, 0.9, 1.0)   # sharp: every token near the cut carries far more than the band
    logits, seen = _case(p)
    ref = SC.ref_sample64(logits, seen, p)
    assert not ref.ambiguous.any()   # the case: no token within the band of the cut
    order = np.argsort(-ref.z.astype(np.float64), kind="stable")
    n = int(ref.support.sum())
    assert ref.support[order[:n]].all() and not ref.support[order[n:]].any()
    early, late = ref.support.copy(), ref.support.copy()
    early[order[n - 1]] = False
    late[order[n]] = True
    _rejects(SC.emulate_weights(logits, seen, p, support=early), ref)
    _rejects(SC.emulate_weights(logits, seen, p, support=late), ref)


def test_comparator_rejects_wrong_step_and_sorted_order_draw():
    p = SC.Params(1.3, 0, 1.0, 1.0)   # flat: two different draws practically never pick the same token
    logits, seen = _case(p)
    ref = SC.ref_sample64(logits, seen, p)
    w = SC.emulate_weights(logits, seen, p)
    n_step = n_sorted = 0
    for step in range(8):
        good = SC.draw_from_weights(w, SEED, step, 0)
        for bad, which in ((SC.draw_from_weights(w, SEED, step + 1, 0), "step"), (SC.draw_from_weights(w, SEED, step, 0, sorted_order=True), "sorted")):
            if bad != good:
                _rejects(w, ref, token=bad, seed=SEED, step=step, row=0)
                n_step += which == "step"
                n_sorted += which == "sorted"
    assert n_step >= 7 and n_sorted >= 7


def test_draw_is_proportional_to_the_weights():
    w = np.array([-1, 3 << 40, 0, 1 << 40, -1, 4 << 40])
    n = 4000
    cnt = np.bincount([SC.draw_from_weights(w, 7, s, 0) for s in range(n)], minlength=6) / n
    assert cnt[0] == cnt[2] == cnt[4] == 0
    assert np.abs(cnt[[1, 3, 5]] - np.array([3, 1, 4]) / 8).max() < 0.03   # 4 sigma of a binomial with n = 4000


# ------------------------------------------------------------------------------------------------ ABI and Python surface
def test_header_declares_and_library_exports_sample_rows():
    from lhrs_bot_amd import _lib

    protos = _lib.parse_header()
    assert "lhrs_sample_rows" in protos
    restype, args = protos["lhrs_sample_rows"]
    assert len(args) == 16
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "lhrs_sample_rows" in set(re.findall(r" T (lhrs_\w+)", exported))
    assert _lib.load().lhrs_abi_version() == 1


def _call(lib, V=32000, mode=0, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, n=1):
    # no pointer is touched before the arguments are accepted: NULL everywhere
    return lib.lhrs_sample_rows(None, V, None, n, V, mode, temperature, top_k, top_p, penalty, None, 0, None, 0, None, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(top_p=0.0), b"top_p"),
    (dict(V=32769), b"V=32769"),
    (dict(V=0), b"V=0"),
    (dict(penalty=1.05), b"seen"),
    (dict(penalty=0.0), b"repetition_penalty"),
    (dict(temperature=0.0), b"temperature"),
    (dict(n=0), b"n=0"),
])
def test_rejected_sample_call_reports_error_without_gpu(kw, msg):
    from lhrs_bot_amd import _lib

    lib = _lib.load()
    st = _call(lib, **kw)
    assert st == -1 and msg in lib.lhrs_last_error(), lib.lhrs_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(st, "sample_rows")


def test_generate_signature_has_the_sampler_keywords():
    from lhrs_bot_amd.text import TextModal

    for fn in (TextModal.generate, TextModal._generate):
        sig = inspect.signature(fn).parameters
        assert sig["sampler"].default == "torch" and sig["seed"].default is None and sig["repetition_penalty"].default == 1.0


def test_cli_has_the_sampler_arguments():
    sys.path.insert(0, ROOT)
    import cli_qa

    cfg = cli_qa.parse_option([])
    assert cfg.sampler == "torch" and cfg.repetition_penalty == 1.0
    cfg = cli_qa.parse_option(["--sampler", "device", "--repetition-penalty", "1.05", "--seed", "7"])
    assert cfg.sampler == "device" and cfg.repetition_penalty == 1.05 and cfg.seed == 7
    with pytest.raises(SystemExit):
        cli_qa.parse_option(["--sampler", "nope"])
