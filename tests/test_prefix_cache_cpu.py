"""generation.match_prefix (which part of a cached conversation a new prompt reuses) against the table and the brute-force count of
tests/prefix_cache_cases.py, and the exactness of the kv8 dequantisation that tests/test_prefix_cache_gpu.py relies on.  No GPU."""
import inspect

import pytest

import prefix_cache_cases as pcc
from lhrs_bot_amd import generation
from lhrs_bot_amd.text import IMAGE_TOKEN_INDEX, TextModal
from lhrs_bot_amd.unibind import UniBind


def test_the_placeholder_is_the_image_token_index():
    assert generation.IMAGE_PLACEHOLDER == IMAGE_TOKEN_INDEX == pcc.IMG


@pytest.mark.parametrize("NI", pcc.NIS)
@pytest.mark.parametrize("case", pcc.CASES, ids=[c[0].replace(" ", "_") for c in pcc.CASES])
def test_match_prefix_case(case, NI):
    name, cached, new, same, tokens, pos = case
    got = generation.match_prefix(list(cached), list(new), NI, same)
    assert got == (tokens, pos(NI)), name
    assert got[1] == pcc.positions(new[:got[0]], NI) == pcc.brute(cached, new, NI, same), name


@pytest.mark.parametrize("NI", pcc.NIS)
def test_match_prefix_random_pairs_against_the_expanded_sequences(NI):
    pairs = pcc.random_pairs(200, seed=NI)
    assert len(pairs) == 200
    seen = set()
    for cached, new, same in pairs:
        tokens, pos = generation.match_prefix(list(cached), list(new), NI, same)
        assert pos == pcc.brute(cached, new, NI, same), (cached, new, same)
        assert pos == pcc.positions(new[:tokens], NI) and cached[:tokens] == new[:tokens], (cached, new, same)
        assert not pcc.inside_block(new, NI, pos), (cached, new, same)
        assert pos < pcc.positions(new, NI) or not new, (cached, new, same)      # one position is left to prefill
        seen.add((pos == 0, pcc.IMG in new[:tokens], same))
    assert len(seen) >= 5                                                        # the draw reaches: nothing / text only / the block, both ways


def test_match_prefix_changes_neither_list():
    cached, new = [1, pcc.IMG, 5], [1, pcc.IMG, 5, 6]
    generation.match_prefix(cached, new, 4, True)
    assert cached == [1, pcc.IMG, 5] and new == [1, pcc.IMG, 5, 6]


def test_dequantised_products_are_exact_in_fp32_and_bf16():
    """e4m3 value (at most 4 significant bits) x 2^(byte - 127): the float64 product, its fp32 value and its bf16 rounding are one number"""
    assert pcc.exact_products() == 254 * len(pcc.BYTES)


def test_prefix_cache_is_a_named_parameter_of_every_generate():
    for fn in (TextModal.generate, generation.generate_rows):
        p = inspect.signature(fn).parameters
        assert "prefix_cache" in p and p["prefix_cache"].default is None, fn.__qualname__
    assert "prefix_cache" in inspect.getdoc(UniBind.generate)
    assert callable(TextModal.new_prefix_cache) and callable(UniBind.new_prefix_cache)


def test_check_rejects_on_the_host_and_changes_nothing():
    import torch
    m = TextModal(device="cpu", layers=2, dim=256, ff=512, heads=2, vocab=128, max_pos=512)
    pc = m.new_prefix_cache("bf16", 64)
    pc.ids, pc.length = [1, pcc.IMG, 5], 6
    ids = torch.tensor([[1, pcc.IMG, 5, 6]])
    assert pc.check(m, ids, None, 1, None, 10, 4) == [1, pcc.IMG, 5, 6] == pc.check(m, ids, torch.ones_like(ids), 1, "bf16", 57, 4)
    other = TextModal(device="cpu", layers=0, dim=256, ff=512, heads=2, vocab=128, max_pos=512)
    for match, args in ((r"shape \(2, 4\)", (m, ids.repeat(2, 1), None, 1, None, 10, 4)),
                        ("num_beams=3", (m, ids, None, 3, None, 10, 4)),
                        ("hides 2 positions", (m, ids, torch.tensor([[0, 0, 1, 1]]), 1, None, 10, 4)),
                        ("2 <image> placeholders", (m, torch.tensor([[1, pcc.IMG, pcc.IMG, 6]]), None, 1, None, 10, 4)),
                        ("kv_cache='fp8' disagrees", (m, ids, None, 1, "fp8", 10, 4)),
                        ("another model", (other, ids, None, 1, None, 10, 4)),
                        (r"prompt \(7\) \+ max_new_tokens \(58\) exceeds the 64 positions", (m, ids, None, 1, None, 58, 4)),
                        (r"prompt \(4\) \+ max_new_tokens \(61\)", (m, ids, None, 1, None, 61, None))):
        with pytest.raises(ValueError, match=match):
            pc.check(*args)
        assert (pc.ids, pc.length, pc.caches) == ([1, pcc.IMG, 5], 6, None)


def test_prefix_cache_construction_on_the_host():
    m = TextModal(device="cpu", layers=2, dim=256, ff=512, heads=2, vocab=128, max_pos=512)
    pc = m.new_prefix_cache()
    assert (pc.kv_cache, pc.max_positions, pc.caches, pc.ids, pc.length, pc.image_embedding, pc.last_reused, pc.last_prefilled) == \
        ("bf16", 512, None, [], 0, None, 0, 0)
    assert m.new_prefix_cache("fp8", 64).max_positions == 64
    with pytest.raises(ValueError, match="int4"):
        m.new_prefix_cache("int4")
    with pytest.raises(ValueError, match="513"):
        m.new_prefix_cache("bf16", 513)
    m64 = TextModal(device="cpu", layers=0, dim=256, ff=512, heads=4, vocab=128, max_pos=512)      # head_dim 64
    with pytest.raises(ValueError, match="head_dim"):
        m64.new_prefix_cache("fp8")
