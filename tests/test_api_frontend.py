"""The Python front end (eigenexa_amd/api.py, eigenexa_amd/_lib.py) against a recording fake of the library: which entry
each of the 19 solver wrappers calls, with which arguments after the ctypes conversion of ``_lib.SIGNATURES``, what it
does with the status, what it returns, and what it refuses before or instead of calling.  CPU only: neither the built
library nor a GPU is needed.  A device tensor is a stub whose class claims to come from ``torch``, which is all that
``api._is_torch`` looks at."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import eigenexa_amd as ee
from c_header import all_prototypes
from eigenexa_amd import _lib, api

N, NVEC, LDA, LDB, LDZ, NB = 6, 5, 7, 8, 9, 3     # all different: a transposed argument shows
IL, IU, VL, VU = 2, 4, -1.5, 2.5
WLEN, ZCOLS = 5, 4                                # entries of w, columns of z: a value window's default mmax is their minimum
M_OUT, IL_OUT = 3, 2                              # what the fake writes through the m and il pointers
MIXED = "must all be host arrays or all be device tensors"
ON_GPU = "torch tensors must live on the GPU \\(use numpy for host arrays\\)"
F_ORDER = "Fortran \\(column-major\\) order required, as in the reference"

# wrapper -> (kind of argument list, entry, complex?, quiet statuses, name in the warnings)
WRAPPERS = {
    "eigen_sx": ("solve", "eigx_sx", False, (0, -5), "eigen_sx"),
    "eigen_s": ("solve", "eigx_s", False, (0, -5), "eigen_s"),
    "eigen_h": ("solve", "eigx_h", True, (0, -5), "eigen_h"),
    "eigen_sx_bc": ("bc2", "eigx_solve_bc", False, (0, -5), "eigen_sx"),
    "eigen_s_bc": ("bc1", "eigx_solve_bc", False, (0, -5), "eigen_s"),
    "eigen_sx_range": ("range", "eigx_sx_range", False, (0, -5), "eigen_sx_range"),
    "eigen_s_range": ("range", "eigx_s_range", False, (0, -5), "eigen_s_range"),
    "eigen_h_range": ("range", "eigx_h_range", True, (0, -5), "eigen_h_range"),
    "eigen_sx_range_v": ("range_v", "eigx_sx_range_v", False, (0, -5, -9), "eigen_sx_range_v"),
    "eigen_s_range_v": ("range_v", "eigx_s_range_v", False, (0, -5, -9), "eigen_s_range_v"),
    "eigen_h_range_v": ("range_v", "eigx_h_range_v", True, (0, -5, -9), "eigen_h_range_v"),
    "eigen_s_batch": ("batch", "eigx_s_batch", False, (0, -5, -6), "eigen_s_batch"),
    "eigen_h_batch": ("batch", "eigx_h_batch", True, (0, -5, -6), "eigen_h_batch"),
    "KMATH_EIGEN_GEV": ("gev", "eigx_gev", False, (0, -7), "KMATH_EIGEN_GEV"),
    "KMATH_EIGEN_GEV_RANGE": ("gev_range", "eigx_gev_range", False, (0, -5, -7), "KMATH_EIGEN_GEV_RANGE"),
    "KMATH_EIGEN_GEV_RANGE_V": ("gev_range_v", "eigx_gev_range_v", False, (0, -5, -7, -9), "KMATH_EIGEN_GEV_RANGE_V"),
    "KMATH_EIGEN_HGEV": ("gev", "eigx_hgev", True, (0, -5, -7), "KMATH_EIGEN_HGEV"),
    "KMATH_EIGEN_HGEV_RANGE": ("gev_range", "eigx_hgev_range", True, (0, -5, -7), "KMATH_EIGEN_HGEV_RANGE"),
    "KMATH_EIGEN_HGEV_RANGE_V": ("gev_range_v", "eigx_hgev_range_v", True, (0, -5, -7, -9), "KMATH_EIGEN_HGEV_RANGE_V"),
}
ALL = sorted(WRAPPERS)
INDEX_WINDOWS = [w for w in ALL if WRAPPERS[w][0] in ("range", "gev_range")]
VALUE_WINDOWS = [w for w in ALL if WRAPPERS[w][0] in ("range_v", "gev_range_v")]
BATCHES = [w for w in ALL if WRAPPERS[w][0] == "batch"]
WITH_BLOCKS = [w for w in ALL if WRAPPERS[w][0] in ("solve", "bc1", "bc2", "range", "range_v")]
UPPER_CASED = INDEX_WINDOWS + VALUE_WINDOWS + BATCHES      # the others that take a mode pass it on as given
SIDES = ["host", "device"]
S_BATCH_3D_TENSOR = ("eigen_s_batch", "host", "z")         # left to test_s_batch_takes_a_3d_tensor_in_a_host_call_as_its_sibling_does


def test_the_table_covers_the_public_solver_wrappers():
    assert len(ALL) == 19 and all(callable(getattr(ee, w)) for w in ALL)


# ------------------------------------------------------------------------------------------------ the fakes
class FakeTensor:
    """what the wrappers look at of a torch tensor; like one it holds the column-major image, so the shape is reversed"""
    _next = 0x7000000

    def __init__(self, dtype, shape, is_cuda=True):
        self.dtype, self.shape, self.ndim, self.is_cuda = dtype, tuple(shape), len(shape), is_cuda
        FakeTensor._next += 0x10000
        self._ptr = FakeTensor._next

    def numel(self):
        return math.prod(self.shape)

    def data_ptr(self):
        return self._ptr


FakeTensor.__module__ = "torch.fake"


class FakeLib:
    """every name of ``_lib.SIGNATURES`` as a ctypes callback with the table's types, so the real conversion of the
    arguments runs; a call is recorded as (name, arguments) with the two int pointers of the value windows replaced by
    'm' and 'il' after M_OUT and IL_OUT were written through them"""

    def __init__(self, events):
        self.events, self.calls, self.status = events, [], 0

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        restype, argtypes = _lib.SIGNATURES[name]

        def recorder(*args):
            seen, out = [], iter((("m", M_OUT), ("il", IL_OUT)))
            for x, t in zip(args, argtypes):
                if t == C.POINTER(C.c_int):
                    label, x[0] = next(out)
                    seen.append(label)
                else:
                    seen.append(x)
            self.events.append(name)
            self.calls.append((name, tuple(seen)))
            return self.status

        fn = C.CFUNCTYPE(restype, *argtypes)(recorder)
        fn.restype, fn.argtypes = restype, list(argtypes)
        self.__dict__[name] = fn
        return fn


class Stream:
    def __init__(self, events):
        self.events = events

    def synchronize(self):
        self.events.append("sync")


@pytest.fixture
def lib(monkeypatch):
    """the fake library behind ``_lib.load``, ``eigen_init`` taken as called, torch's current stream recorded"""
    events = []
    fake = FakeLib(events)

    def load():
        events.append("load")
        return fake

    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setitem(api._state, "initialized", True)
    monkeypatch.setitem(api._state, "last_status", 12345)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: Stream(events))
    return fake


@pytest.fixture
def no_lib(monkeypatch):
    def boom():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setitem(api._state, "last_status", 12345)


def make(dtype, shape, side, is_cuda=True):
    """an array of Fortran shape ``shape`` on ``side``"""
    if side == "host":
        return np.zeros(shape, dtype=dtype, order="F")
    return FakeTensor(getattr(torch, np.dtype(dtype).name), tuple(shape)[::-1], is_cuda)


def addr(x):
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def arrays(wrapper, side):
    kind, _, cplx, _, _ = WRAPPERS[wrapper]
    dt = np.complex128 if cplx else np.float64
    if kind == "batch":
        return dict(a=make(dt, (LDA, N, NB), side), w=make(np.float64, (N, NB), side), z=make(dt, (LDZ, N, NB), side))
    arr = dict(a=make(dt, (LDA, N), side), w=make(np.float64, (WLEN,), side), z=make(dt, (LDZ, ZCOLS), side))
    if kind.startswith("gev"):
        arr["b"] = make(dt, (LDB, N), side)
    return arr


def plan(wrapper, arr, md=b"A", mf=48, mb=128, mmax=ZCOLS):
    """the positional arguments of a call of ``wrapper`` on the arrays ``arr``, and the tuple that must reach the C entry"""
    kind = WRAPPERS[wrapper][0]
    a, b, w, z = (arr.get(k) for k in "abwz")
    A, B, W, Z = (addr(arr.get(k)) for k in "abwz")
    if kind == "solve":
        return (N, NVEC, a, LDA, w, z, LDZ), (N, NVEC, A, LDA, W, Z, LDZ, mf, mb, md)
    if kind in ("bc1", "bc2"):
        return (N, NVEC, a, LDA, w, z, LDZ, NB), (int(kind[2]), N, NVEC, A, LDA, W, Z, LDZ, NB, mf, mb, md)
    if kind == "range":
        return (N, IL, IU, a, LDA, w, z, LDZ), (N, IL, IU, A, LDA, W, Z, LDZ, mf, mb, md)
    if kind == "range_v":
        return (N, VL, VU, a, LDA, w, z, LDZ), (N, VL, VU, mmax, "m", "il", A, LDA, W, Z, LDZ, mf, mb, md)
    if kind == "batch":
        return (N, NB, a, LDA, w, z, LDZ), (N, NB, A, LDA, LDA * N, W, N, Z, LDZ, LDZ * N, md, None)
    if kind == "gev":
        return (N, a, LDA, b, LDB, w, z, LDZ), (N, A, LDA, B, LDB, W, Z, LDZ)
    if kind == "gev_range":
        return (N, IL, IU, a, LDA, b, LDB, w, z, LDZ), (N, IL, IU, A, LDA, B, LDB, W, Z, LDZ, md)
    assert kind == "gev_range_v"
    return (N, VL, VU, a, LDA, b, LDB, w, z, LDZ), (N, VL, VU, mmax, "m", "il", A, LDA, B, LDB, W, Z, LDZ, md)


def entry_of(wrapper, side):
    return WRAPPERS[wrapper][1] + ("_dev" if side == "device" else "")


def events_of(wrapper, side):
    return ["load"] + (["sync"] if side == "device" else []) + [entry_of(wrapper, side)]


def returned(wrapper, status):
    return (M_OUT, IL_OUT) if wrapper in VALUE_WINDOWS and status in (0, -9) else None


# ------------------------------------------------------------------------------------------------ entry and arguments
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", ALL)
def test_defaults_reach_the_entry(lib, capsys, wrapper, side):
    """the entry for the side, the whole argument tuple with the defaults (block sizes 48 / 128, mode 'A', a value window's
    mmax, the batch strides), one stream synchronisation between the load and the call on the device side only"""
    args, expected = plan(wrapper, arrays(wrapper, side))
    assert getattr(ee, wrapper)(*args) == returned(wrapper, 0)
    assert lib.calls == [(entry_of(wrapper, side), expected)]
    assert lib.events == events_of(wrapper, side)
    assert api.last_status() == 0
    assert capsys.readouterr().err == ""


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", ALL)
def test_given_arguments_reach_the_entry(lib, wrapper, side):
    """block sizes as given; a lower-case mode upper-cased by the window and batch wrappers and passed on as it is by the
    others; a missing z arrives as a null pointer"""
    kind = WRAPPERS[wrapper][0]
    arr = arrays(wrapper, side)
    kw = {}
    if kind != "gev":
        kw["mode"] = "n"
        if kind not in ("solve", "bc1", "bc2"):
            arr["z"] = None
    if wrapper in WITH_BLOCKS:
        kw.update(m_forward=32, m_backward=64)
    args, expected = plan(wrapper, arr, md=b"N" if wrapper in UPPER_CASED else b"n", mf=32, mb=64, mmax=WLEN)
    getattr(ee, wrapper)(*args, **kw)
    assert lib.calls == [(entry_of(wrapper, side), expected)]


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", [w for w in ALL if w != "KMATH_EIGEN_HGEV"])
def test_missing_arrays_arrive_as_null(lib, wrapper, side):
    """w and z of None go to the library as null pointers where no check of the wrapper's own needs them (mode 'N')"""
    kind = WRAPPERS[wrapper][0]
    arr = arrays(wrapper, side)
    arr["z"] = None
    if kind not in ("range_v", "gev_range_v", "batch"):                # those need w for mmax / refuse a missing w
        arr["w"] = None
    args, expected = plan(wrapper, arr, md=b"N", mmax=WLEN)
    getattr(ee, wrapper)(*args, **({} if kind == "gev" else {"mode": "N"}))
    assert lib.calls == [(entry_of(wrapper, side), expected)]


@pytest.mark.parametrize("which, side", [(k, "host") for k in "abwz"] + [(k, "device") for k in "bwz"])   # a decides the side
def test_hgev_passes_a_missing_array_as_null(lib, capsys, which, side):
    # ALLOWED DIFFERENCE 1 (fails on the parent): KMATH_EIGEN_HGEV had lost the `x is None` branch of its siblings and
    # raised AttributeError (ValueError in a device call); now None reaches eigx_hgev[_dev] as null, which answers -2
    # (EIGX_ERR_BAD_ARG)
    arr = arrays("KMATH_EIGEN_HGEV", side)
    arr[which] = None
    args, expected = plan("KMATH_EIGEN_HGEV", arr)
    lib.status = -2
    assert ee.KMATH_EIGEN_HGEV(*args) is None
    assert lib.calls == [(entry_of("KMATH_EIGEN_HGEV", side), expected)]
    assert api.last_status() == -2
    assert capsys.readouterr().err == "Warning: KMATH_EIGEN_HGEV returned without computing (status -2)\n"


# ------------------------------------------------------------------------------------------------ status and return value
@pytest.mark.parametrize("status", [0, -5, -6, -7, -9, -3])
@pytest.mark.parametrize("wrapper", ALL)
def test_status_warning_and_return_value(lib, capsys, wrapper, status):
    _, _, _, quiet, name = WRAPPERS[wrapper]
    lib.status = status
    args, _ = plan(wrapper, arrays(wrapper, "host"))
    assert getattr(ee, wrapper)(*args) == returned(wrapper, status)
    assert api.last_status() == status
    warning = "" if status in quiet else f"Warning: {name} returned without computing (status {status})\n"
    assert capsys.readouterr().err == warning


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", ALL)
def test_not_initialised(lib, monkeypatch, capsys, wrapper, side):
    """before eigen_init: status -1, nothing called, the stream not synchronised, nothing printed, None returned"""
    monkeypatch.setitem(api._state, "initialized", False)
    args, _ = plan(wrapper, arrays(wrapper, side))
    assert getattr(ee, wrapper)(*args) is None
    assert api.last_status() == -1
    assert lib.calls == [] and lib.events == ["load"]
    assert capsys.readouterr().err == ""


# ------------------------------------------------------------------------------------------------ value windows
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", VALUE_WINDOWS)
def test_value_window_mmax(lib, wrapper, side):
    """default: the entries of w, further limited by the columns of a 2-D z (z.shape[1] of a numpy array, z.shape[0] of a
    device tensor); mode 'N' does not look at z; a given mmax is passed through"""
    arr = arrays(wrapper, side)
    args, expected = plan(wrapper, arr, mmax=ZCOLS)
    getattr(ee, wrapper)(*args)
    wide = dict(arr, z=make(np.complex128 if WRAPPERS[wrapper][2] else np.float64, (LDZ, WLEN + 2), side))
    args_wide, expected_wide = plan(wrapper, wide, mmax=WLEN)
    getattr(ee, wrapper)(*args_wide)
    _, expected_n = plan(wrapper, arr, md=b"N", mmax=WLEN)
    getattr(ee, wrapper)(*args, mode="N")
    _, expected_2 = plan(wrapper, arr, mmax=2)
    getattr(ee, wrapper)(*args, mmax=2)
    assert [c[1] for c in lib.calls] == [expected, expected_wide, expected_n, expected_2]


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", VALUE_WINDOWS)
def test_value_window_count_mode(lib, wrapper, side):
    """mode 'C' passes mmax 0 whatever was given and accepts w and z of None"""
    arr = dict(arrays(wrapper, side), w=None, z=None)
    args, expected = plan(wrapper, arr, md=b"C", mmax=0)
    assert getattr(ee, wrapper)(*args, mode="c") == (M_OUT, IL_OUT)
    assert getattr(ee, wrapper)(*args, mode="C", mmax=7) == (M_OUT, IL_OUT)
    assert lib.calls == [(entry_of(wrapper, side), expected)] * 2


# ------------------------------------------------------------------------------------------------ batch wrappers
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", BATCHES)
def test_batch_arguments(lib, wrapper, side):
    arr = arrays(wrapper, side)
    a, w, z = arr["a"], arr["w"], arr["z"]
    A, W, Z = addr(a), addr(w), addr(z)
    info = make(np.int32, (NB,), side)
    fn = getattr(ee, wrapper)
    fn(N, NB, a, LDA, w, None, None, mode="N")                                     # no z, no ldz: zeros and a null
    fn(N, NB, a, LDA, w, z, LDZ, mode="N")                                         # mode 'N' never passes z on
    fn(N, NB, a, LDA, w, z, LDZ, info=info)                                        # info as an address
    fn(N, NB, a, LDA, w, z, LDZ, stride_a=50, ldw=N + 1, stride_z=60)              # given strides pass through
    fn(N, NB, a, LDA, w, z, LDZ, "a", info, 50, N + 1, 60)                         # the same by position
    assert [c[1] for c in lib.calls] == [
        (N, NB, A, LDA, LDA * N, W, N, None, 0, 0, b"N", None),
        (N, NB, A, LDA, LDA * N, W, N, None, LDZ, LDZ * N, b"N", None),
        (N, NB, A, LDA, LDA * N, W, N, Z, LDZ, LDZ * N, b"A", addr(info)),
        (N, NB, A, LDA, 50, W, N + 1, Z, LDZ, 60, b"A", None),
        (N, NB, A, LDA, 50, W, N + 1, Z, LDZ, 60, b"A", addr(info)),
    ]
    assert {c[0] for c in lib.calls} == {entry_of(wrapper, side)}


@pytest.mark.parametrize("wrapper", BATCHES)
def test_batch_info_must_be_int32_on_the_side_of_a(lib, wrapper):
    fn = getattr(ee, wrapper)
    for side, other in (("host", "device"), ("device", "host")):
        args, _ = plan(wrapper, arrays(wrapper, side))
        with pytest.raises(ValueError, match="a, w, z, info " + MIXED):
            fn(*args, info=make(np.int32, (NB,), other))
        wrong = "info: int32 required" if side == "host" else "info: int32 GPU tensor required"
        with pytest.raises(ValueError, match=wrong):
            fn(*args, info=make(np.int64, (NB,), side))
    args, _ = plan(wrapper, arrays(wrapper, "device"))
    with pytest.raises(ValueError, match="info: int32 GPU tensor required"):
        fn(*args, info=make(np.int32, (NB,), "device", is_cuda=False))
    assert lib.calls == []


# ------------------------------------------------------------------------------------------------ refused before the library
def _refused(capsys, wrapper, args, kw, text):
    api._state["last_status"] = 12345
    assert getattr(ee, wrapper)(*args, **kw) is None
    assert api.last_status() == -2, (args, kw)
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith(f"Warning: {WRAPPERS[wrapper][4]}: {text} (n="), err
    return err


@pytest.mark.parametrize("wrapper", INDEX_WINDOWS)
def test_bad_index_windows(no_lib, capsys, wrapper):
    """il < 1, iu > n, il > iu, n <= 0, no number, a mode outside A / N, a missing z in mode A"""
    arr = arrays(wrapper, "host")
    gev = WRAPPERS[wrapper][0] == "gev_range"
    rows = [(N, 0, 3, {}), (N, 2, N + 1, {}), (N, 5, 4, {}), (0, 1, 1, {}), (-1, 1, 1, {}), (N, "x", 3, {}), (N, None, 3, {}),
            (N, 1, 3, {"mode": "X"}), (N, 1, 3, {"mode": "C"}), (N, 1, 3, {"z": None})]
    for n, il, iu, change in rows:
        kw = {k: v for k, v in change.items() if k == "mode"}
        a, w, z = arr["a"], arr["w"], change.get("z", arr["z"])
        args = (n, il, iu, a, LDA, arr["b"], LDB, w, z, LDZ) if gev else (n, il, iu, a, LDA, w, z, LDZ)
        err = _refused(capsys, wrapper, args, kw, "invalid window / mode")
        mode = kw.get("mode", "A")
        assert err == f"Warning: {WRAPPERS[wrapper][4]}: invalid window / mode (n={n}, il={il}, iu={iu}, mode={mode!r})\n"


@pytest.mark.parametrize("wrapper", VALUE_WINDOWS)
def test_bad_value_windows(no_lib, capsys, wrapper):
    """vl >= vu, a NaN bound, n <= 0, no number, a mode outside A / N / C, no room, a missing w or z"""
    arr = arrays(wrapper, "host")
    gev = WRAPPERS[wrapper][0] == "gev_range_v"
    nan = float("nan")
    rows = [(N, 1.0, 1.0, {}), (N, 2.0, 1.0, {}), (N, nan, 1.0, {}), (N, 0.0, nan, {}), (0, VL, VU, {}), (N, "x", VU, {}),
            (N, VL, VU, {"mode": "X"}), (N, VL, VU, {"mmax": 0}), (N, VL, VU, {"mmax": -1}), (N, VL, VU, {"w": None}),
            (N, VL, VU, {"z": None}), (N, VL, VU, {"w": None, "mode": "N"})]
    for n, vl, vu, change in rows:
        kw = {k: v for k, v in change.items() if k in ("mode", "mmax")}
        a, w, z = arr["a"], change.get("w", arr["w"]), change.get("z", arr["z"])
        args = (n, vl, vu, a, LDA, arr["b"], LDB, w, z, LDZ) if gev else (n, vl, vu, a, LDA, w, z, LDZ)
        _refused(capsys, wrapper, args, kw, "invalid window / mode")
    args = (N, 2.0, 1.0, arr["a"], LDA, arr["b"], LDB, arr["w"], arr["z"], LDZ) if gev else \
        (N, 2.0, 1.0, arr["a"], LDA, arr["w"], arr["z"], LDZ)
    err = _refused(capsys, wrapper, args, {"mode": "n"}, "invalid window / mode")
    assert err == f"Warning: {wrapper}: invalid window / mode (n={N}, vl=2.0, vu=1.0, mmax=None, mode='n')\n"


@pytest.mark.parametrize("wrapper", BATCHES)
def test_bad_batch_arguments(no_lib, capsys, wrapper):
    arr = arrays(wrapper, "host")
    ok = dict(n=N, batch=NB, a=arr["a"], lda=LDA, w=arr["w"], z=arr["z"], ldz=LDZ)
    bad = [dict(n=0), dict(n=-1), dict(batch=-1), dict(lda=N - 1), dict(ldw=N - 1), dict(stride_a=LDA * N - 1), dict(ldz=N - 1),
           dict(stride_z=LDZ * N - 1), dict(z=None), dict(a=None), dict(w=None), dict(mode="X"), dict(mode="C"), dict(n="x"),
           dict(ldz=None)]
    for change in bad:
        _refused(capsys, wrapper, (), {**ok, **change}, "invalid arguments")
    err = _refused(capsys, wrapper, (), {**ok, "lda": N - 1, "mode": "a"}, "invalid arguments")
    assert err == (f"Warning: {wrapper}: invalid arguments (n={N}, batch={NB}, lda={N - 1}, ldw={N}, ldz={LDZ}, "
                   f"stride_a={(N - 1) * N}, stride_z={LDZ * N}, mode='a')\n")


# ------------------------------------------------------------------------------------------------ ValueErrors
def _arrays_named(wrapper):
    return [k for k in "abwz" if k in arrays(wrapper, "host")]


def _raises(lib, wrapper, arr, message):
    args, _ = plan(wrapper, arr)
    with pytest.raises(ValueError, match=message):
        getattr(ee, wrapper)(*args)
    assert lib.calls == []


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("wrapper", ALL)
def test_wrong_dtype(lib, wrapper, side):
    """every array in turn: float64 for w and for the real wrappers, complex128 for a, b, z of the complex ones"""
    cplx = WRAPPERS[wrapper][2]
    for k in _arrays_named(wrapper):
        arr = arrays(wrapper, side)
        good = arr[k]
        want = "complex128" if cplx and k != "w" else "float64"
        for wrong in (np.float32, np.float64 if want == "complex128" else np.complex128):
            shape = good.shape if side == "host" else good.shape[::-1]
            _raises(lib, wrapper, dict(arr, **{k: make(wrong, shape, side)}), f"^{k}: {want} required$")


@pytest.mark.parametrize("wrapper", ALL)
def test_c_ordered_host_arrays(lib, wrapper):
    """a 2-D numpy array in C order; for the batch wrappers a 3-D one"""
    for k in _arrays_named(wrapper):
        arr = arrays(wrapper, "host")
        if arr[k].ndim == 1:
            continue
        if wrapper in BATCHES and arr[k].ndim == 2:
            continue                                                               # w(ldw, batch) with ldw = n is checked below
        _raises(lib, wrapper, dict(arr, **{k: np.zeros(arr[k].shape, dtype=arr[k].dtype, order="C")}), f"^{k}: {F_ORDER}$")
    if wrapper in BATCHES:
        arr = arrays(wrapper, "host")
        _raises(lib, wrapper, dict(arr, w=np.zeros((N, NB), order="C")), f"^w: {F_ORDER}$")


@pytest.mark.parametrize("wrapper", ALL)
def test_host_and_device_arguments_mixed(lib, wrapper):
    # ALLOWED DIFFERENCE 2: the names in front of the sentence ("a, w, z" in some wrappers, "a, b, w, z" in others) may
    # become one form; the sentence itself is matched
    for side, other in (("host", "device"), ("device", "host")):
        for k in _arrays_named(wrapper)[1:]:                                       # a decides the side
            if (wrapper, side, k) == S_BATCH_3D_TENSOR:
                continue
            arr = arrays(wrapper, side)
            arr[k] = arrays(wrapper, other)[k]
            _raises(lib, wrapper, arr, MIXED + "$")


@pytest.mark.parametrize("wrapper", ALL)
def test_torch_tensor_that_is_not_on_the_gpu(lib, wrapper):
    """the real wrappers say that torch tensors must live on the GPU, whichever argument it is and whatever the side; the
    complex ones count such a tensor as a mixed call"""
    cplx = WRAPPERS[wrapper][2]
    for side in SIDES:
        for k in _arrays_named(wrapper):
            if (wrapper, side, k) == S_BATCH_3D_TENSOR:
                continue
            arr = arrays(wrapper, side)
            good = arrays(wrapper, "device")[k]
            arr[k] = FakeTensor(good.dtype, good.shape, is_cuda=False)
            _raises(lib, wrapper, arr, MIXED + "$" if cplx else f"^{k}: {ON_GPU}$")


def test_s_batch_takes_a_3d_tensor_in_a_host_call_as_its_sibling_does(lib):
    # A THIRD DIFFERENCE, of the kind of the first (fails on the parent): eigen_s_batch asked a torch z of a host call for
    # numpy's ``flags`` and raised AttributeError; eigen_h_batch had the guard.  With one body both raise the ValueError.
    host = arrays("eigen_s_batch", "host")
    _raises(lib, "eigen_s_batch", dict(host, z=arrays("eigen_s_batch", "device")["z"]), MIXED + "$")
    _raises(lib, "eigen_s_batch", dict(host, z=FakeTensor(torch.float64, (NB, N, LDZ), is_cuda=False)), f"^z: {ON_GPU}$")


def test_checks_come_in_todays_order(lib):
    """of two faults the first one of today's order is reported: a real wrapper looks at a tensor's place, then its dtype,
    then the side of the call; a complex one at the side first; a host array's side comes before its dtype and its order"""
    f32 = make(np.float32, (LDA, N), "device")
    off_gpu_f32 = FakeTensor(torch.float32, (N, LDA), is_cuda=False)
    c_order_f32 = np.zeros((LDA, N), dtype=np.float32)
    host, dev = arrays("eigen_s", "host"), arrays("eigen_s", "device")
    _raises(lib, "eigen_s", dict(host, z=f32), "^z: float64 required$")
    _raises(lib, "eigen_s", dict(host, z=off_gpu_f32), f"^z: {ON_GPU}$")
    _raises(lib, "eigen_s", dict(dev, z=c_order_f32), MIXED + "$")
    _raises(lib, "eigen_s", dict(host, z=c_order_f32), "^z: float64 required$")
    host, dev = arrays("eigen_h", "host"), arrays("eigen_h", "device")
    _raises(lib, "eigen_h", dict(host, z=f32), MIXED + "$")
    _raises(lib, "eigen_h", dict(dev, z=off_gpu_f32), MIXED + "$")
    _raises(lib, "eigen_h", dict(dev, z=c_order_f32), MIXED + "$")
    _raises(lib, "eigen_h", dict(host, z=c_order_f32), "^z: complex128 required$")
    # the first faulty argument in the order a, (b,) w, z is the one named
    host = arrays("KMATH_EIGEN_GEV", "host")
    _raises(lib, "KMATH_EIGEN_GEV", dict(host, b=c_order_f32, z=c_order_f32), "^b: float64 required$")
    # a batch wrapper looks at the order of all its 3-D arrays before any dtype
    host = arrays("eigen_s_batch", "host")
    _raises(lib, "eigen_s_batch", dict(host, a=np.zeros((LDA, N, NB), dtype=np.float32, order="F"),
                                       z=np.zeros((LDZ, N, NB))), f"^z: {F_ORDER}$")


def test_arguments_are_checked_after_the_stream_is_synchronised(lib):
    """the order load -> init check -> side -> synchronise -> addresses: a device call with a bad array has synchronised"""
    for wrapper in ALL:
        del lib.events[:]
        arr = arrays(wrapper, "device")
        arr["w"] = make(np.float32, (WLEN,), "device")
        _raises(lib, wrapper, arr, "^w: float64 required$")
        assert lib.events == ["load", "sync"], wrapper


# ------------------------------------------------------------------------------------------------ the ctypes table
# eigenexa_amd/_lib.py's table as it stood before its argument lists were named: "name restype:argtypes" with i c_int,
# l c_int64, d c_double, c c_char, p c_void_p, s c_char_p, I / L / D POINTER(c_int / c_int64 / c_double)
SIGNATURES_BEFORE = """
eigx_init i:i
eigx_init_multi i:iiipc
eigx_get_rccl_unique_id i:p
eigx_get_device_count i:
eigx_get_comm i:IIII
eigx_comm_seconds d:
eigx_comm_info i:si
eigx_rccl_selftest i:
eigx_free i:
eigx_get_version i:Iss
eigx_get_procs i:III
eigx_get_id i:III
eigx_get_errinfo i:L
eigx_get_matdims i:iIIiic
eigx_matdims_for_grid i:iiiiicII
eigx_held_bytes l:
eigx_held_bytes_named l:s
eigx_transpose_plan i:iiiiiiIIIII
eigx_memory_internal l:iiiii
eigx_loop_start i:iii
eigx_loop_end i:iii
eigx_translate_l2g i:iii
eigx_translate_g2l i:iii
eigx_owner_node i:iii
eigx_owner_index i:iii
eigx_sx i:iipippiiic
eigx_s i:iipippiiic
eigx_sx_dev i:iipippiiic
eigx_s_dev i:iipippiiic
eigx_solve_bc i:iiipippiiiic
eigx_solve_bc_dev i:iiipippiiiic
eigx_numroc i:iiii
eigx_h i:iipippiiic
eigx_h_dev i:iipippiiic
eigx_set_grid_dims i:ii
eigx_band_reduce_dev i:ipippiii
eigx_band_dc_dev i:iippiippi
eigx_gev i:ipipippi
eigx_gev_dev i:ipipippi
eigx_hgev i:ipipippi
eigx_hgev_dev i:ipipippi
eigx_sx_range i:iiipippiiic
eigx_s_range i:iiipippiiic
eigx_sx_range_dev i:iiipippiiic
eigx_s_range_dev i:iiipippiiic
eigx_sx_range_v i:iddiIIpippiiic
eigx_s_range_v i:iddiIIpippiiic
eigx_sx_range_v_dev i:iddiIIpippiiic
eigx_s_range_v_dev i:iddiIIpippiiic
eigx_gev_range_v i:iddiIIpipippic
eigx_gev_range_v_dev i:iddiIIpipippic
eigx_band_count_dev i:ippiiipp
eigx_band_bisect_range_dev i:iiippiip
eigx_band_eigvec_dev i:iippiipppi
eigx_range_info i:IID
eigx_range_timers i:D
eigx_gev_range i:iiipipippic
eigx_gev_range_dev i:iiipipippic
eigx_chol_dev i:ipi
eigx_trsm_upper_dev i:ciipipi
eigx_gev_reduce_dev i:ipipi
eigx_hgev_range i:iiipipippic
eigx_hgev_range_dev i:iiipipippic
eigx_h_range i:iiipippiiic
eigx_h_range_dev i:iiipippiiic
eigx_h_range_v i:iddiIIpippiiic
eigx_h_range_v_dev i:iddiIIpippiiic
eigx_hgev_range_v i:iddiIIpipippic
eigx_hgev_range_v_dev i:iddiIIpipippic
eigx_s_batch i:iipilpipilcp
eigx_s_batch_dev i:iipilpipilcp
eigx_h_batch i:iipilpipilcp
eigx_h_batch_dev i:iipilpipilcp
eigx_zchol_dev i:ipi
eigx_ztrsm_upper_dev i:ciipipi
eigx_hgev_reduce_dev i:ipipi
eigx_band_bisect_dev i:ippiip
eigx_trbak_dev i:iipipipiii
eigx_dgemm_dev i:cciiidpipidpii
eigx_dgemm_gather_dev i:cciiidpipidpipp
eigx_get_timers i:D
eigx_profile i:i
eigx_profile_read i:D
eigx_profile_read_kinds i:Di
eigx_tune i:ii
eigx_device_synchronize i:
eigx_malloc_dev p:l
eigx_free_dev i:p
eigx_memcpy_h2d i:ppl
eigx_memcpy_d2h i:ppl
"""
LETTERS = {"i": C.c_int, "l": C.c_int64, "d": C.c_double, "c": C.c_char, "p": C.c_void_p, "s": C.c_char_p,
           "I": C.POINTER(C.c_int), "L": C.POINTER(C.c_int64), "D": C.POINTER(C.c_double)}


def test_the_ctypes_table_is_what_it_was():
    """same names in the same order, equal values element for element"""
    before = [line.split() for line in SIGNATURES_BEFORE.split("\n") if line]
    assert [name for name, _ in before] == list(_lib.SIGNATURES)
    for name, sig in before:
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is LETTERS[sig[0]], name
        assert isinstance(argtypes, list) and len(argtypes) == len(sig) - 2, name
        assert all(t is LETTERS[s] for t, s in zip(argtypes, sig[2:])), name


def _kinds_of(ctype_text):
    """the ctypes types that may stand for a parameter or return type of the header"""
    t = ctype_text.replace("const ", "").replace(" *", "*")
    plain = {"char": C.c_char, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    typed = {"int*": C.POINTER(C.c_int), "double*": C.POINTER(C.c_double), "int64_t*": C.POINTER(C.c_int64)}
    if t in plain:
        return (plain[t],)
    if t in typed:
        return (typed[t], C.c_void_p)
    assert t.endswith("*"), ctype_text
    return (C.c_void_p, C.c_char_p)


def test_every_prototype_of_the_header_matches_the_ctypes_table():
    """for every symbol of include/eigenexa_amd.h: the number of parameters, the kind of each, the return type"""
    protos = all_prototypes()
    assert set(protos) == set(_lib.SIGNATURES) and len(protos) >= 90
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype in (_kinds_of(ret)[:1] if "*" not in ret else (C.c_void_p,)), name
        assert len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            ctype_text = p.rsplit(" ", 1)[0]                                       # "const double* a_dev" -> "const double*"
            assert t in _kinds_of(ctype_text), (name, p, t)
