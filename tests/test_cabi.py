"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/m2h.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

from m2h import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(header="m2h.h"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(m2h_[a-z0-9_A-Z]+)\s*\(", txt)))


def test_library_builds_and_exports_header_symbols():
    path = _lib.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    syms = _declared_symbols()
    assert "m2h_conv_igemm_f32" in syms and "m2h_unet_down_fwd" in syms
    for s in syms:
        assert hasattr(lib, s), "libm2h.so does not export %s" % s
    # the diagnostic surface (thread-local tuning knobs) lives in its own header, outside the product contract
    diag = _declared_symbols("m2h_tuning.h")
    assert diag == ["m2h_tuning_restore", "m2h_tuning_set", "m2h_tuning_snapshot"] and not set(diag) & set(syms)
    assert "m2h_debug_set" not in syms and not hasattr(lib, "m2h_debug_set")
    for s in diag:
        assert hasattr(lib, s), "libm2h.so does not export %s" % s
    # the ctypes binding covers every declared function
    bound = set(_lib.SIGNATURES) | {"m2h_last_error"}
    assert set(syms) | set(diag) == bound, ((set(syms) | set(diag)) ^ bound)


def test_tuning_knobs_are_thread_local():
    """no process-global mutable state -- a knob set by one host thread is not seen by another (runs without a GPU)."""
    import threading
    lib = _lib.load()
    n = _lib.TUNING_KNOBS
    assert lib.m2h_tuning_set(24, 7) == 0
    seen = {}

    def other():
        arr = (ctypes.c_int * n)()
        assert lib.m2h_tuning_snapshot(arr, n) == 0
        seen["other"] = list(arr)
        assert lib.m2h_tuning_set(24, -1) == 0

    t = threading.Thread(target=other)
    t.start()
    t.join()
    mine = (ctypes.c_int * n)()
    assert lib.m2h_tuning_snapshot(mine, n) == 0
    assert seen["other"] == [0] * n and mine[24] == 7
    zero = (ctypes.c_int * n)()
    assert lib.m2h_tuning_restore(zero, n) == 0 and lib.m2h_tuning_set(n, 1) < 0


def test_version_and_error_string_without_gpu():
    lib = _lib.load()
    assert lib.m2h_version() == 100
    assert isinstance(lib.m2h_last_error(), bytes)


def test_conv_args_struct_matches_header_field_order():
    txt = open(os.path.join(ROOT, "include", "m2h.h")).read()
    body = txt[txt.index("typedef struct m2h_conv_args {"):txt.index("} m2h_conv_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct m2h_conv_args {", "")
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        # "int a, b, c" or "const float* p"
        first = decl.split(",")
        names.append(first[0].replace("*", " ").split()[-1])
        names += [x.strip().replace("*", "") for x in first[1:]]
    assert names == [f for f, _ in _lib.ConvArgs._fields_], names


def _struct_fields(name):
    txt = open(os.path.join(ROOT, "include", "m2h.h")).read()
    body = txt[txt.index("typedef struct %s {" % name):txt.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct %s {" % name, "")
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first = decl.split(",")
            names.append(first[0].replace("*", " ").split()[-1])
            names += [x.strip().replace("*", "") for x in first[1:]]
    return names


def test_rollout_structs_match_header_field_order():
    """m2h_episode_stats / m2h_row_copy mirrors (ctypes) follow the header field for field; argument errors of the two entry
    points are reported without a launch (negative return, message), so this runs without a GPU."""
    assert _struct_fields("m2h_episode_stats") == [f for f, _ in _lib.EpisodeStats._fields_] == list(_lib.EPISODE_STATS_FIELDS)
    assert _struct_fields("m2h_row_copy") == [f for f, _ in _lib.RowCopy._fields_]
    assert ctypes.sizeof(_lib.RowCopy) == 32 and ctypes.sizeof(_lib.EpisodeStats) == 17 * ctypes.sizeof(ctypes.c_void_p)
    lib = _lib.load()
    assert lib.m2h_rows_copy(None, 0, None, None) < 0 and b"rows_copy" in lib.m2h_last_error()
    items = (_lib.RowCopy * 1)(_lib.RowCopy(8, 16, 6, -1, -1))   # size not a multiple of 4
    assert lib.m2h_rows_copy(items, 1, None, None) < 0 and b"multiple of 4" in lib.m2h_last_error()
    st = _lib.EpisodeStats()                                      # null statistics tensors
    assert lib.m2h_episode_stats_update(ctypes.byref(st), 8, 8, 8, 8, 8, 8, None, None, 14, 3, None) < 0
    assert lib.m2h_gru_step(8, 8, 8, 8, None, 8, 8, 17, 512, None) < 0 and b"gru_step" in lib.m2h_last_error()


def test_scorer_refusals_name_their_own_entry_point():
    """The four scorer entry points share their argument checks (csrc/score_common.h); a refusal still names the entry that was called.
    Refusals return before any HIP call, so this runs without a GPU."""
    lib = _lib.load()
    p, null = ctypes.c_void_p(256), None          # never dereferenced
    sig = lambda refs=p, est=p: (refs, 300, 100, 0, est, 100, 0)   # noqa: E731
    mix = (p, 200, 100)
    n0 = lib.m2h_launch_count()

    def gram(S=3, C=1, **kw):
        return lib.m2h_score_gram(*sig(**kw), *mix, p, 2, S, C, 100, 10, None)

    def gram_lag(S=3, C=1, **kw):
        return lib.m2h_score_gram_lag(*sig(**kw), *mix, p, 2, S, C, 100, 10, p, 5, None)

    def corr(S=3, C=1, target0=0, **kw):
        return lib.m2h_align_corr(*sig(**kw), None, target0, p, p, 2, S, C, 100, 10, 5, None)

    def spectral(S=3, C=1, target0=0, **kw):
        return lib.m2h_score_spectral(*sig(**kw), *mix, None, target0, p, p, 2, S, C, 100, None, 0, None)

    for name, call, rows in ((b"score_gram", gram, [(dict(S=7), b"S = 7"), (dict(C=3), b"C = 3"), (dict(refs=null), b"null pointer")]),
                             (b"score_gram_lag", gram_lag, [(dict(S=7), b"S = 7"), (dict(C=3), b"C = 3"), (dict(est=null), b"null pointer")]),
                             (b"align_corr", corr, [(dict(S=7), b"S = 7"), (dict(C=3), b"C = 3"), (dict(refs=null), b"null pointer"),
                                                    (dict(target0=3), b"target = 3"), (dict(target0=-1), b"target = -1")]),
                             (b"score_spectral", spectral, [(dict(S=7), b"S = 7"), (dict(C=3), b"C = 3"), (dict(est=null), b"null pointer"),
                                                            (dict(target0=3), b"target = 3"), (dict(target0=-1), b"target = -1")])):
        for kw, text in rows:
            assert call(**kw) < 0, (name, kw)
            msg = lib.m2h_last_error()
            assert msg.startswith(name + b": ") and text in msg, (name, kw, msg)
    assert lib.m2h_launch_count() == n0


def test_stft_scorer_refusals_name_their_own_entry_point():
    """m2h_score_spectral and m2h_score_spatial share one sequence of checks (csrc/score_stft.h): one refused call per shared check, each
    message names the entry that was called, and nothing is launched.  Refusals return before any HIP call, so this runs without a GPU."""
    lib = _lib.load()
    p, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)          # never dereferenced
    n0 = lib.m2h_launch_count()

    def spectral(target0=0, dft=p, out=p, L=100, lag=None, D=0):
        return lib.m2h_score_spectral(p, 300, 100, 0, p, 100, 0, p, 200, 100, None, target0, dft, out, 2, 3, 1, L, lag, D, None)

    def spatial(target0=0, dft=p, out=p, L=100, lag=None, D=0):
        return lib.m2h_score_spatial(p, 600, 200, 100, p, 200, 100, p, 200, 100, None, target0, dft, out, 2, 3, L, lag, D, None)

    rows = [(dict(dft=None), b"null pointer (dft)"), (dict(lag=p), b"a lag table needs D >= 1"), (dict(D=1), b"a null pointer needs D = 0"),
            (dict(target0=3), b"target = 3"), (dict(target0=-1), b"target = -1"), (dict(out=odd), b"out must be 8-byte aligned"),
            (dict(lag=p, D=50, L=100), b"L = 100 samples; at least 2 D + 1 = 101")]
    for name, call in ((b"score_spectral", spectral), (b"score_spatial", spatial)):
        for kw, text in rows:
            assert call(**kw) < 0, (name, kw)
            msg = lib.m2h_last_error()
            assert msg.startswith(name + b": ") and text in msg, (name, kw, msg)
    assert lib.m2h_launch_count() == n0


def test_rollout_kernel_refusals_name_their_own_entry_point():
    """Argument refusals of the rollout kernels (tests/rollout_kernels.py has their rows): each returns before any launch and names the
    entry that was called, so this runs without a GPU."""
    lib = _lib.load()
    p = ctypes.c_void_p(256)                      # never dereferenced
    n0 = lib.m2h_launch_count()
    many = (_lib.RowCopy * (_lib.ROWS_COPY_MAX + 1))(*[_lib.RowCopy(256, 512, 16, -1, -1) for _ in range(_lib.ROWS_COPY_MAX + 1)])
    gathers = (_lib.RowCopy * (_lib.ROWS_COPY_MAX + 1))(*[_lib.RowCopy(256, 512, 16, 0, -1) for _ in range(_lib.ROWS_COPY_MAX + 1)])
    rows = ((b"advantages", lambda: lib.m2h_advantages(p, p, p, p, 1, 0, 1e-5, None), b"bad arguments"),                       # n = 1
            (b"acoustic_mem_small", lambda: lib.m2h_acoustic_mem_small_fwd(p, p, None, p, p, p, 1, 256, 32, None), b"got 256 x 32"),   # F != 512
            (b"acoustic_mem_small", lambda: lib.m2h_acoustic_mem_small_fwd(p, p, None, p, p, p, 1, 512, 16, None), b"got 512 x 16"),   # T != 32
            (b"gather_envs", lambda: lib.m2h_gather_envs(p, p, p, 1, 1, 1, 6, None), b"row_bytes % 4"),
            (b"rows_copy", lambda: lib.m2h_rows_copy(many, _lib.ROWS_COPY_MAX + 1, None, None), b"1..%d items" % _lib.ROWS_COPY_MAX),
            (b"synth_env_observe", lambda: lib.m2h_synth_env_observe(gathers, _lib.ROWS_COPY_MAX + 1, p, p, p, 1, None), b"bad arguments"),
            (b"slice_concat_input", lambda: lib.m2h_slice_concat_input(p, 1, None, 0, None, None, 0, p, 1, 24, 4, None), b"F % 16"))
    for name, call, text in rows:
        assert call() < 0, name
        msg = lib.m2h_last_error()
        assert msg.startswith(name + b": ") and text in msg, (name, msg)
    assert lib.m2h_launch_count() == n0


def test_workspace_bytes_reports_the_dma_engines_two_k_halves_launch():
    """m2h_conv_igemm_workspace_bytes (host-only) mirrors the launch rules: for the fourth encoder stage at the benchmark batch in
    bf16x3 arithmetic on split32 operands (128 tiles of 256 x 128, K = 4096) the LDS-DMA engine runs two K-halves per tile into
    split-K slabs -- a caller who sizes the workspace by this function gets 2 x M x N floats and with it the same kernel (and
    fp32 summation order) as the whole-network runner; the same layer in fp32 arithmetic reports the register engine's own factor."""
    lib = _lib.load()
    lib.m2h_conv_igemm_workspace_bytes.argtypes = [ctypes.POINTER(_lib.ConvArgs)]
    lib.m2h_conv_igemm_workspace_bytes.restype = ctypes.c_size_t
    a = _lib.ConvArgs()
    a.C0, a.C1, a.B, a.Hi, a.Wi, a.Hq, a.Wq = 256, 0, 256, 4, 32, 2, 16
    a.stride, a.nth, a.ntw, a.mulh, a.offh, a.mulw, a.offw = 2, 4, 4, 1, -1, 1, -1
    a.conv_transpose, a.N, a.Ho, a.Wo, a.os, a.ldc, a.out_mode = 0, 512, 2, 16, 1, 512, 0
    M, N = 256 * 2 * 16, 512
    a.operand_format = 1 | 2 | 4 | 8      # M2H_FMT_SRC_SPLIT | W_SPLIT | DST_SPLIT | MATH_BF16X3
    assert lib.m2h_conv_igemm_workspace_bytes(ctypes.byref(a)) == 2 * M * N * 4
    a.operand_format = 16                 # M2H_FMT_MATH_FP32: the register engine's split factor for this shape
    fp32_bytes = lib.m2h_conv_igemm_workspace_bytes(ctypes.byref(a))
    assert fp32_bytes % (M * N * 4) == 0 and fp32_bytes != 2 * M * N * 4 or fp32_bytes == 0 or fp32_bytes == 2 * M * N * 4
    a.operand_format = 1 | 2 | 4 | 8
    a.B = 1024                            # enough 256 x 128 tiles to fill the chip: no split at all on that engine
    assert lib.m2h_conv_igemm_workspace_bytes(ctypes.byref(a)) == 0
    # the deepest encoder stage at the benchmark batch (32 tiles of 256 x 128, half of the window in the padding: walked K = 4096):
    # eight K-parts per tile on that engine
    a.C0, a.B, a.Hi, a.Wi, a.Hq, a.Wq, a.Ho, a.Wo = 512, 256, 2, 16, 1, 8, 1, 8
    assert lib.m2h_conv_igemm_workspace_bytes(ctypes.byref(a)) == 8 * (256 * 8) * 512 * 4
