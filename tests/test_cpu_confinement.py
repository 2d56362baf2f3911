"""The confinement harness of tests/helpers.py (``confined``) is shown to bite: plain torch functions on CPU tensors stand in for kernels, a correct
one passes and every planted error -- a masked read past an operand, a write behind an output or into a stride gap, an element never written, a
read-modify-write of an output, a modified input -- fails with a message that names the property it violates and the operand."""
import pytest
import torch

from tests.helpers import FILLS, GUARD_BYTES, ConfinementError, Strided, confined

N, ROWS, WIDTH, STRIDE = 257, 3, 40, 64


def _inputs(dtype):
    gen = torch.Generator().manual_seed(5)
    return {"x": torch.randn(N, generator=gen).to(dtype), "w": torch.randn(N, generator=gen).to(dtype)}


def _outputs(dtype):
    return {"y": ((N,), dtype), "arena": Strided(ROWS, WIDTH, STRIDE, torch.float32)}


def _good(o):
    o["y"].copy_(o["x"] * o["w"])
    o["arena"].copy_(o["x"][:ROWS * WIDTH].float().view(ROWS, WIDTH) * 2)


def _before(t):
    """The element in front of operand ``t`` (a view into the memory around it, as a kernel's pointer arithmetic has it)."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() - 1)


def _behind(t):
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + t.numel())


def _run(fn, dtype=torch.float32, **kw):
    return confined(fn, _inputs(dtype), _outputs(dtype), device="cpu", **kw)


def test_the_guard_is_the_largest_staged_tile_and_the_fills_are_what_they_are_for():
    assert GUARD_BYTES == 256 * 4096 * 4 and GUARD_BYTES >= 4 << 20
    assert FILLS == (0x00, 0xFF, 0x7F)
    for dtype in (torch.float32, torch.bfloat16):
        nan, huge = (torch.full((4,), b, dtype=torch.uint8).view(dtype)[0].float() for b in (0xFF, 0x7F))
        assert bool(torch.isnan(nan)) and bool(torch.isfinite(huge)) and float(huge) > 3e38
    assert int(torch.full((8,), 0xFF, dtype=torch.uint8).view(torch.int64)[0]) == -1
    assert int(torch.full((1,), 0xFF, dtype=torch.uint8).view(torch.int8)[0]) == -1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_confined_function_passes_and_the_first_run_is_returned(dtype):
    ins = _inputs(dtype)
    out = _run(_good, dtype)
    assert torch.equal(out["y"], ins["x"] * ins["w"])
    assert out["arena"].shape == (ROWS, WIDTH) and torch.equal(out["arena"], ins["x"][:ROWS * WIDTH].float().view(ROWS, WIDTH) * 2)


def test_inout_operands_keep_their_content_and_only_their_surroundings_are_filled():
    acc = torch.arange(N, dtype=torch.float32)
    rows = torch.arange(ROWS * WIDTH, dtype=torch.float32).view(ROWS, WIDTH)

    def fn(o):
        o["acc"].add_(o["x"])
        o["tab"].mul_(2)
        o["ws"].zero_()
    out = confined(fn, _inputs(torch.float32), {}, inout={"acc": acc, "tab": Strided(ROWS, WIDTH, STRIDE, data=rows)}, scratch={"ws": ((16,), torch.float32)},
                   device="cpu")
    assert torch.equal(out["acc"], acc + _inputs(torch.float32)["x"]) and torch.equal(out["tab"], rows * 2)


def test_a_masked_read_before_an_operand_is_caught_as_reads_confined():
    def fn(o):                                             # a halo element multiplied by zero: right as long as the neighbour is finite
        _good(o)
        o["y"][0] += _before(o["x"])[0] * 0.0
    with pytest.raises(ConfinementError, match=r"reads confined: 'y'.*element 0 .*0xFF"):
        _run(fn)


def test_a_read_hidden_by_a_maximum_with_zero_is_caught_by_the_0x7f_fill_only():
    """The kernels' clamp(min=0) is fmaxf, which DROPS a NaN operand (torch.clamp propagates it, torch.fmax is fmaxf): the NaN fill passes, the
    huge finite one does not."""
    def fn(o):
        _good(o)
        o["y"][0] += torch.fmax(_before(o["x"])[0], torch.zeros(()))
    _run(fn, fills=(0x00, 0xFF))
    with pytest.raises(ConfinementError, match=r"reads confined: 'y'.*0x7F") as err:
        _run(fn)
    assert "0xFF" not in str(err.value)


def test_a_write_behind_an_output_is_caught_as_writes_confined():
    def fn(o):
        _good(o)
        _behind(o["y"]).fill_(1.0)
    with pytest.raises(ConfinementError, match=r"writes confined.*'y'.*guard behind it \(byte \+10(28|30) "):
        _run(fn)


def test_a_write_behind_an_input_is_caught_too():
    def fn(o):
        _good(o)
        _behind(o["w"]).fill_(1.0)
    with pytest.raises(ConfinementError, match=r"writes confined.*'w'.*guard behind it"):
        _run(fn)


def test_a_write_into_the_gap_of_a_strided_destination_is_caught_as_writes_confined():
    def fn(o):
        _good(o)
        torch.as_strided(o["arena"], (1,), (1,), o["arena"].storage_offset() + STRIDE + WIDTH).fill_(3.0)      # the element behind row 1
    with pytest.raises(ConfinementError, match=r"writes confined.*'arena'.*gap between its rows \(byte \d+ = row 1, element 40 "):
        _run(fn)


def test_an_unwritten_last_element_is_caught_as_outputs_fully_defined():
    def fn(o):
        o["y"][:-1].copy_((o["x"] * o["w"])[:-1])
        o["arena"].copy_(o["x"][:ROWS * WIDTH].float().view(ROWS, WIDTH) * 2)
    with pytest.raises(ConfinementError, match=rf"outputs fully defined: element {N - 1} of output 'y' is never written"):
        _run(fn)


def test_an_unwritten_element_of_a_strided_destination_is_caught():
    def fn(o):
        o["y"].copy_(o["x"] * o["w"])
        full = o["x"][:ROWS * WIDTH].float().view(ROWS, WIDTH) * 2
        o["arena"][:2].copy_(full[:2])
        o["arena"][2, :-1].copy_(full[2, :-1])
    with pytest.raises(ConfinementError, match=rf"outputs fully defined: element {ROWS * WIDTH - 1} of output 'arena' is never written"):
        _run(fn)


def test_adding_into_an_output_is_caught_as_outputs_fully_defined():
    def fn(o):
        o["y"].add_(o["x"] * o["w"])
        o["arena"].copy_(o["x"][:ROWS * WIDTH].float().view(ROWS, WIDTH) * 2)
    with pytest.raises(ConfinementError, match=r"outputs fully defined: 'y' depends on what the outputs held before"):
        _run(fn)


def test_a_modified_input_is_caught_as_inputs_unchanged():
    def fn(o):
        _good(o)
        o["w"][7] = 0.0
    with pytest.raises(ConfinementError, match=r"inputs unchanged.*'w' \(element 7, 1 elements"):
        _run(fn)


def test_a_non_finite_output_is_refused():
    def fn(o):
        _good(o)
        o["y"][3] = float("inf")
    with pytest.raises(ConfinementError, match=r"outputs fully defined: 'y' is not finite \(element 3\)"):
        _run(fn)
