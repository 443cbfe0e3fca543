"""The C ABI refuses every defective operating-point call with the code it has always
refused it with: tests/golden/abi_refusals.json (recorded from the library before the host
side of mhe_gn.hip was folded onto one validation path; tests/golden/gen_abi_refusals.py)
replayed against the built library.  Single defects and pairs of two, eleven entry points,
six dims; a few thousand calls that return at once.

The calls pass fake pointers, so the replay runs only where no GPU is visible: a regression
that lets a defective call through must fail at its first HIP call, never enqueue kernels
on those pointers on a card other work shares."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_abi_refusals as gen  # noqa: E402

from mhe import _lib  # noqa: E402

pytestmark = pytest.mark.skipif(not gen.no_gpu_visible(),
                                reason="a GPU is visible: defective calls with fake pointers are replayed only "
                                       "where a call let through cannot enqueue kernels on them")


def test_recorded_refusals_replay_with_equal_codes():
    with open(gen.OUT) as f:
        want = json.load(f)
    lib = _lib.load()
    got, built, kept = gen.record(lib, strict=False)
    print(f"{built} calls built, {kept} refusals ({want['built']} / {want['kept']} recorded)")
    assert want["kept"] > 5000 and (built, kept) == (want["built"], want["kept"])
    assert list(got) == list(want["cases"]) == list(gen.FNS)
    bad = []
    for fn in gen.FNS:
        assert list(got[fn]) == list(want["cases"][fn]) == list(gen.DIMS)
        for dn, w in want["cases"][fn].items():
            g = got[fn][dn]
            names = w["defects"]
            assert g["defects"] == names, (fn, dn)  # the cases themselves are the recorded ones
            if g["base"] != w["base"]:
                bad.append((fn, dn, (), w["base"], g["base"]))
            for i, (a, b) in enumerate(zip(w["single"], g["single"])):
                if a != b:
                    bad.append((fn, dn, (names[i],), a, b))
            for i, (wr, gr) in enumerate(zip(w["pair"], g["pair"])):
                assert len(wr) == len(gr) == len(names) - 1 - i
                for k, (a, b) in enumerate(zip(wr, gr)):
                    if a != b:
                        bad.append((fn, dn, (names[i], names[i + 1 + k]), a, b))
    for fn, dn, chosen, a, b in bad[:40]:
        print(f"{fn} on {dn} with {chosen}: recorded {a}, now {b}")
    assert not bad, f"{len(bad)} calls are refused with another code than recorded (or let through)"
    assert want["changed"] == []  # no double defect answers with its other defect's code
