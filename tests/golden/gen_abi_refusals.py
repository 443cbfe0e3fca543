"""Writes tests/golden/abi_refusals.json: the code every defective call of the C ABI's
operating-point entry points is refused with, recorded from a libmhe.so built from the
commit a host-side change starts from (MHE_LIB selects the library):

    MHE_LIB=/path/to/parent/libmhe.so python tests/golden/gen_abi_refusals.py

tests/test_abi_refusals.py replays the file against the built library: a host-side refactor
must refuse every call with the code it was refused with before, and before any launch.

Calls pass fake non-NULL pointers (FAKE, as tests/test_cov_host.py), so this runs only where
no GPU is visible: a call the library lets through fails at its first HIP call instead of
enqueuing kernels on those pointers.  Every (entry point, dims) gets its defects one at a
time and every pair of two; a call without defects is recorded only where it is itself a
refusal (an entry point that does not take those dims).  Every recorded call must be a
refusal: no MHE_ERR_HIP, and MHE_OK only with batch = 0.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "nlp-filter_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from mhe import _lib  # noqa: E402

OUT = os.path.join(HERE, "abi_refusals.json")
OK, ERR_HIP = 0, -3
FAKE = ctypes.c_void_p(4096)  # a non-NULL pointer no check dereferences
BATCH = 2
_EQ = (ctypes.c_int32 * 2)(0, 1)  # one equality row v[0] = v[1]; kept alive here


def no_gpu_visible():
    import torch
    return torch.cuda.device_count() == 0


# ------------------------------------------------------------------ dims
def _c2(has_prior=0, n_eq=0):
    d = _lib.MheDims()  # van der Pol + full_state, N = 100: register path, linear rows (p = 2)
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 100, 2, 1, 2, 101, 0, 5, 1, 10.0
    d.has_prior = has_prior
    if n_eq:
        d.n_eq, d.eq_idx = 1, ctypes.cast(_EQ, ctypes.POINTER(ctypes.c_int32))
    return d


def _c3():
    d = _lib.MheDims()  # gnss_pos_and_bias + pseudorange, N = 200: large path, scalar nonlinear rows
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 200, 5, 3, 1, 2412, 3, 6, 2, 200.0
    for i in range(4):
        d.meas_idx[i] = i
    return d


def _mixed(path=_lib.PATH_AUTO):
    d = _lib.MheDims()  # two receivers + mixed rows with two extra variables, N = 10
    d.N, d.n, d.m, d.p, d.M, d.q, d.dyn_model, d.meas_model, d.T = 10, 10, 6, 1, 30, 14, 8, 5, 5.0
    d.n_extra, d.force_large = 2, path
    return d


DIMS = {
    "c2": _c2,
    "c2_prior": lambda: _c2(has_prior=1),
    "c3": _c3,
    "mixed_extra": _mixed,                                   # large path, n_extra > 0
    "fused_general": lambda: _mixed(_lib.PATH_FUSED_GENERAL),  # k_gn_general's dims
    "c2_eq": lambda: _c2(n_eq=1),                            # an equality row: large path
}

STRUCT_FNS = ("mhe_solve", "mhe_state_cov", "mhe_arrival", "mhe_kkt_cov", "mhe_kkt_arrival", "mhe_assemble_at")
FNS = STRUCT_FNS + ("mhe_assemble", "mhe_assemble_ws", "mhe_assemble_kkt_ws", "mhe_chol_solve", "mhe_chol_solve_ws")
WS_FNS = STRUCT_FNS + ("mhe_assemble_ws", "mhe_assemble_kkt_ws", "mhe_chol_solve_ws")
SCRATCH_FNS = ("mhe_state_cov", "mhe_arrival", "mhe_kkt_cov", "mhe_kkt_arrival")
ARGS_PTRS = ("X0", "X_out", "Z0", "Z_out", "U", "Y", "PAR", "x0", "cost_out", "iters_out", "status_out")


class Call:
    """One call of ``fn`` on the dims ``dname`` with every argument valid; defects edit it."""

    def __init__(self, lib, fn, dname):
        self.fn, self.d = fn, DIMS[dname]()
        a = self.a = _lib.MheSolveArgs()
        a.batch, a.max_iter, a.tol = BATCH, 5, 1e-9
        for k in ARGS_PTRS:
            setattr(a, k, FAKE)
        self.ws_bytes = lib.mhe_workspace_bytes(self.d, BATCH)
        self.big = self.ws_bytes > 0
        a.workspace, a.workspace_bytes = (FAKE if self.big else None), self.ws_bytes
        self.n_query = 1
        self.scratch_bytes = lib.mhe_cov_scratch_bytes(self.d, BATCH, 1)
        self.scratch = FAKE if self.scratch_bytes else None
        self.args_null = False
        # the call's own pointers: cov_opt / covz are optional outputs
        self.p = dict(cbuf=FAKE, PhiQ=FAKE, cov=FAKE, covz=None, cov_opt=None, status=FAKE, x_arr=FAKE, Pw_arr=FAKE,
                      H=FAKE, g=FAKE, cost=FAKE, delta=FAKE)

    def required(self):
        """The pointers this call must not pass NULL (given its dims and path)."""
        d, fn, nz = self.d, self.fn, self.d.n_extra > 0
        if fn in ("mhe_chol_solve", "mhe_chol_solve_ws"):
            return ["cbuf", "H", "g", "delta", "status"]
        pt = ["cbuf", "X0"] + ["Y"] * (d.M > 0) + ["U"] * (d.m > 0) + ["PAR"] * (d.q > 0) + ["x0"] * bool(d.has_prior)
        if fn == "mhe_solve":
            return ["args"] + pt + ["X_out", "cost_out", "iters_out", "status_out"] + ["Z0", "Z_out"] * nz
        if fn in ("mhe_state_cov", "mhe_kkt_cov"):
            return ["args"] + pt + ["PhiQ", "cov", "status"] + ["Z0"] * (nz and fn == "mhe_kkt_cov")
        if fn in ("mhe_arrival", "mhe_kkt_arrival"):
            return ["args"] + pt + ["PhiQ", "x_arr", "Pw_arr", "status"] + ["Z0"] * (nz and fn == "mhe_kkt_arrival")
        out = pt + ["H", "g", "cost"] + ["status"] * (self.big and fn != "mhe_assemble")
        if fn == "mhe_assemble_at":
            return ["args"] + out + ["Z0"] * (nz and self.big)
        return out + ["Z0"] * (nz and self.big and fn == "mhe_assemble_kkt_ws")

    def invoke(self, lib):
        d, a, p, fn = self.d, self.a, self.p, self.fn
        ar = None if self.args_null else ctypes.byref(a)
        pos = (a.X0, a.U, a.u_bstride, a.Y, a.PAR, a.par_bstride, a.x0)
        ws = (a.workspace, a.workspace_bytes)
        sc = (self.scratch, self.scratch_bytes)
        if fn == "mhe_solve":
            return lib.mhe_solve(d, p["cbuf"], ar, None)
        if fn == "mhe_state_cov":
            return lib.mhe_state_cov(d, p["cbuf"], ar, p["PhiQ"], self.n_query, p["cov"], p["status"], *sc, None)
        if fn == "mhe_kkt_cov":
            return lib.mhe_kkt_cov(d, p["cbuf"], ar, p["PhiQ"], self.n_query, p["cov"], p["covz"], p["status"], *sc,
                                   None)
        if fn in ("mhe_arrival", "mhe_kkt_arrival"):
            return getattr(lib, fn)(d, p["cbuf"], ar, p["PhiQ"], p["x_arr"], p["Pw_arr"], p["cov_opt"], p["status"],
                                    *sc, None)
        if fn == "mhe_assemble_at":
            return lib.mhe_assemble_at(d, p["cbuf"], ar, p["H"], p["g"], p["cost"], p["status"], None)
        if fn == "mhe_assemble":
            return lib.mhe_assemble(d, p["cbuf"], a.batch, *pos, p["H"], p["g"], p["cost"], None)
        if fn == "mhe_assemble_ws":
            return lib.mhe_assemble_ws(d, p["cbuf"], a.batch, *pos, p["H"], p["g"], p["cost"], p["status"], *ws, None)
        if fn == "mhe_assemble_kkt_ws":
            return lib.mhe_assemble_kkt_ws(d, p["cbuf"], a.batch, a.X0, a.Z0, *pos[1:], p["H"], p["g"], p["cost"],
                                           p["status"], *ws, None)
        if fn == "mhe_chol_solve":
            return lib.mhe_chol_solve(d, p["cbuf"], a.batch, p["H"], p["g"], p["delta"], p["status"], None)
        return lib.mhe_chol_solve_ws(d, p["cbuf"], a.batch, p["H"], p["g"], p["delta"], p["status"], *ws, None)


# ------------------------------------------------------------------ defects
def _null(name):
    def apply(c):
        if name == "args":
            c.args_null = True
        elif name in ARGS_PTRS:
            setattr(c.a, name, None)
        else:
            c.p[name] = None
    return apply


def _set_args(**kw):
    def apply(c):
        for k, v in kw.items():
            setattr(c.a, k, v)
    return apply


def _stale(which):
    def apply(c):
        if which == "args":
            c.a.struct_size -= 8
        else:
            c.d.struct_size -= 4
    return apply


def _set(**kw):
    def apply(c):
        for k, v in kw.items():
            setattr(c, k, v)
    return apply


def _linear(c):
    return c.d.meas_model == 1  # MHE_MEAS_FULL_STATE: the one linear model


def defects(c):
    """[(name, slot, apply)] for the call ``c``: two defects of one slot edit the same argument
    and are never paired."""
    fn, out = c.fn, []
    for name in c.required():
        out.append(("null:" + name, name, _null(name)))
    if fn in STRUCT_FNS:
        out.append(("stale:args", "args_size", _stale("args")))
    out.append(("stale:dims", "dims_size", _stale("dims")))
    out.append(("batch=-1", "batch", _set_args(batch=-1)))
    out.append(("batch=0", "batch", _set_args(batch=0)))
    if fn == "mhe_solve":
        out.append(("max_iter=-1", "max_iter", _set_args(max_iter=-1)))
    if fn in ("mhe_state_cov", "mhe_kkt_cov"):
        out.append(("n_query=0", "n_query", _set(n_query=0)))
    if fn in STRUCT_FNS:
        if _linear(c):  # a linear h folds Rw into the constants; its rows here are p = 2
            out.append(("Rw:linear", "Rw", _set_args(Rw=FAKE)))
            out.append(("meas_delta:p!=1", "meas_delta", _set_args(meas_delta=FAKE)))
        elif fn == "mhe_solve" and c.d.force_large == _lib.PATH_FUSED_GENERAL:
            out.append(("meas_delta:fused", "meas_delta", _set_args(meas_delta=FAKE)))  # k_gn_general has no robust rows
        if not c.d.has_prior:
            out.append(("Pw:no_prior", "Pw", _set_args(Pw=FAKE)))
    if c.big and fn in WS_FNS:
        out.append(("ws:missing", "ws", _set_args(workspace=None)))
        out.append(("ws:short", "ws", _set_args(workspace_bytes=c.ws_bytes - 1)))
    if c.big and fn in SCRATCH_FNS:
        out.append(("scratch:missing", "scratch", _set(scratch=None)))
        out.append(("scratch:short", "scratch", _set(scratch_bytes=c.scratch_bytes - 1)))
    return out


def run(lib, fn, dname, chosen=()):
    """The code of ``fn`` on ``dname`` with the defects named ``chosen``, and the batch passed."""
    c = Call(lib, fn, dname)
    table = {name: apply for name, _, apply in defects(c)}
    for name in chosen:
        table[name](c)
    return c.invoke(lib), c.a.batch


def record(lib, strict=True):
    """{fn: {dims: {"defects": names, "base": code | None, "single": codes, "pair": rows}}} and the
    counts (built, kept).  pair[i][k] is the code of defects i and i + 1 + k together (None: one
    slot).  strict: every recorded call must be a refusal (the generator's own check)."""
    cases, built, kept = {}, 0, 0

    def one(fn, dname, chosen):
        nonlocal built, kept
        rc, batch = run(lib, fn, dname, chosen)
        built += 1
        if not chosen and (rc == ERR_HIP or rc == OK):
            return None  # a valid call went on to its first HIP call: not a refusal, not recorded
        if strict:
            assert rc != ERR_HIP and (rc != OK or batch == 0), \
                f"{fn} on {dname} with {chosen} was let through (rc {rc}): the case is not a defect here"
        kept += 1
        return rc

    for fn in FNS:
        for dname in DIMS:
            ds = defects(Call(lib, fn, dname))
            names = [n for n, _, _ in ds]
            e = {"defects": names, "base": one(fn, dname, ()), "single": [one(fn, dname, (n,)) for n in names]}
            e["pair"] = [[None if ds[i][1] == ds[j][1] else one(fn, dname, (names[i], names[j]))
                          for j in range(i + 1, len(ds))] for i in range(len(ds))]
            cases.setdefault(fn, {})[dname] = e
    return cases, built, kept


def main():
    assert no_gpu_visible(), "fake pointers: run this only where no GPU is visible"
    lib = _lib.load()
    cases, built, kept = record(lib)
    lines = ["{", f' "abi_version": 11, "built": {built}, "kept": {kept},',
             ' "changed": [],', ' "cases": {']
    for i, fn in enumerate(FNS):
        lines.append(f'  "{fn}": {{')
        rows = [f'   "{dn}": ' + json.dumps(cases[fn][dn], separators=(",", ":")) for dn in DIMS]
        lines.append(",\n".join(rows))
        lines.append("  }" + ("," if i + 1 < len(FNS) else ""))
    lines += [" }", "}", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print(f"{OUT}: {built} calls built, {kept} refusals kept, library {_lib.LIB_PATH} ({_lib.lib_digest()})")


if __name__ == "__main__":
    main()
