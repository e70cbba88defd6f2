"""tests/pass_borders.py without a device: its mirrors of cct_jpegls_bound, cct_tiff_bound and cct_png_bound against the
library's host functions, its constants against the source text, and every batch plan against the conditions a plan has
to meet before tests/test_gpu_pass_borders.py spends a gigabyte on it: two passes at least, a short last pass of two
frames at least, planted frames and refusals on both sides of every border, frames that differ from their neighbours,
the rule that cuts, and no frame more than that takes."""
import numpy as np
import pytest

import jpeg_ls_model as jm
import pass_borders as pb
import png_model as pm
import tiff_model as tm

ALL = pb.ENCODER_PLANS + pb.BORDER_PLANS + pb.REFUSED_PASS_PLANS   # built inside the tests, not at collection


def test_the_constants_are_the_source_texts():
    assert pb.JLS_PASS_BYTES == 512 << 20 and pb.TIFF_PASS_BYTES == 512 << 20 and pb.DEFLATE_PASS_BYTES == 1 << 30
    assert pb.JLS_LIMIT_MAX == 64 and pb.JLS_HDR_MAX == 32
    with pytest.raises(AssertionError):
        pb.constant("api_tiff.cpp", "NO_SUCH_CONSTANT")
    with pytest.raises(AssertionError):
        pb.constant("api_jpeg_ls.cpp", r"JLS_\w+")  # JLS_MAX_PIXELS and JLS_PASS_BYTES both match: refused, not guessed


def test_bound_mirrors_equal_the_library():
    from cct_hip import _ffi
    L = _ffi.lib()
    jls = {(p.rows, p.cols, p.params["restart_rows"]) for p in pb.all_plans() if "jpegls" in p.entry}
    jls |= {(r, c, rr) for r in jm.ROWS for c in jm.COLS for rr in jm.RESTARTS + (16, 65535)}
    jls |= {(0, 4, 0), (4, 4, -1), (65535, 65535, 0), (8192, 8192, 16), (8193, 8192, 0), (512, 512, 0), (512, 512, 16)}
    for rows, cols, rr in sorted(jls):
        assert pb.jpegls_bound(rows, cols, rr) == L.cct_jpegls_bound(rows, cols, rr), (rows, cols, rr)
    tiff = {(pb.TIFF_WRITE_SHAPE, 16, (0,)), (pb.TIFF_READ_SHAPE, 16, (0, pb.TIFF_READ_RPS)), ((512, 512), 16, (0, 50)), ((65535, 65535), 16, (0, 1)),
            ((0, 5), 8, (0,)), ((5, 5), 12, (0,))}
    tiff |= {(a.shape, 8 * a.dtype.itemsize, tuple(r or 0 for r in rpss)) for _, a, rpss in tm.raster_cases()}
    for (rows, cols), bits, rpss in sorted(tiff):
        for comp in (1, 5, 8, 7):
            for rps in rpss + (-1,):
                assert pb.tiff_bound(rows, cols, bits, comp, rps) == L.cct_tiff_bound(rows, cols, bits, comp, rps), (rows, cols, bits, comp, rps)
    png = {pb.PNG_SHAPE, (512, 512), (1, 1), (0, 3), (3, 0), (23170, 23170), (23171, 23170), (3, 16500)} | {x.shape for x in pm.cases().values()}
    for rows, cols in sorted(png):
        assert pb.png_bound(rows, cols) == L.cct_png_bound(rows, cols), (rows, cols)


def test_the_uniform_passes_follow_per_pass():
    assert pb._even_passes(7, 3) == [(0, 3), (3, 6), (6, 7)] and pb._even_passes(6, 3) == [(0, 3), (3, 6)] and pb._even_passes(1, 9) == [(0, 1)]
    # what the entry points' comments and the older multi-pass tests say of known shapes
    assert pb.png_encode_per_pass(512, 512, 16) == (1 << 30) // 525056 and pb.png_read_per_pass(512, 512) == (1 << 30) // 524816
    assert pb.jpegls_encode_per_pass(65535, 1024, 0) == 1   # one frame at least
    assert pb.tiff_encode_per_pass(1, 1, 8, 1, 0) == (512 << 20) // (256 + 144)


def test_the_two_cut_rules():
    cut = pb._cut_passes
    assert cut([5] * 7, 10, 1000, 30) == ([(0, 3), (3, 6), (6, 7)], ["rasters", "rasters", "end"])
    assert cut([5] * 7, 10, 12, 1000) == ([(0, 2), (2, 4), (4, 6), (6, 7)], ["files", "files", "files", "end"])
    assert cut([50, 1, 1], 10, 12, 1000) == ([(0, 1), (1, 3)], ["files", "end"])   # a pass holds one file at least
    assert cut([6, 6, 0, 0], 10, 12, 1000)[0] == [(0, 4)]                           # at the limit is inside it
    assert pb.jpegls_decode_passes([1 << 27, 1], 1, 1, 8)[0] == [(0, 1), (1, 2)] and pb.jpegls_decode_passes([(1 << 27) - 1, 1], 1, 1, 8)[0] == [(0, 2)]
    assert pb.tiff_read_passes([1 << 29, 1], 1, 1, 8)[0] == [(0, 1), (1, 2)] and pb.tiff_read_passes([(1 << 29) - 1, 1], 1, 1, 8)[0] == [(0, 2)]


@pytest.mark.parametrize("make", ALL, ids=lambda f: f.__name__)
def test_every_plan_meets_its_conditions(make):
    p = make()
    print(p.describe())
    first, last = p.passes[0], p.passes[-1]
    assert len(p.passes) >= 2 and first[0] == 0 and last[1] == p.n
    assert all(a[1] == b[0] for a, b in zip(p.passes, p.passes[1:]))
    assert 2 <= last[1] - last[0] < first[1] - first[0] == p.per_pass
    assert last[1] - last[0] == p.params["tail"] and p.n == (len(p.passes) - 1) * p.per_pass + p.params["tail"]  # not a frame more than the roles need
    asserted = [i for i, r in p.roles.items() if r != "host:junk"]
    assert p.n - 1 in asserted
    for c0, _ in p.passes[1:]:
        if make in pb.REFUSED_PASS_PLANS:
            continue
        if make in pb.ENCODER_PLANS or p.params.get("rule") == "files":
            assert {c0 - 1, c0, c0 + 1} <= set(asserted)
        else:  # a host refusal and a device refusal on each side, good frames around them
            assert [p.roles.get(i, "").split("/")[0] for i in range(c0 - 3, c0 + 3)] == ["planted", "host:a", "device:a", "device:b", "host:b", "planted"]
    if p.name == "jls_encode":
        c0 = p.passes[1][0]
        assert [p.roles.get(i) for i in range(c0 - 2, c0 + 3)] == ["planted", "overflow", "planted", "overflow", "planted"]
    # a frame a test asserts on differs from both neighbours, and from the frame a dropped c0 would put in its place
    if make in pb.ENCODER_PLANS:
        content = lambda i: pb.raster(p, p.key(i)).tobytes()  # noqa: E731
    else:
        content = lambda i: pb.FILE_OF[p.entry](p, p.key(i))[0]  # noqa: E731
    for i in asserted:
        for j in (i - 1, i + 1, i - p.per_pass, i % p.per_pass):
            if 0 <= j < p.n and j != i:
                assert content(i) != content(j), (i, j)
    assert len({content(k) for k in range(pb.FILLERS)}) == pb.FILLERS
    assert p.host_bytes < 3 * max(pb.JLS_PASS_BYTES, pb.DEFLATE_PASS_BYTES) // 2


def test_encoder_plans_cross_by_their_formula():
    p = pb.jls_encode_plan()
    assert p.per_pass == pb.JLS_PASS_BYTES // (((pb.jpegls_bound(40, 500, 16) + 3) & ~3) + 3 * ((pb.jls_interval_bound(16, 500) + 3) & ~3)) == 1223
    p, pz, pn = pb.tiff_encode_plan(), pb.tiff_encode_deflate_plan(), pb.tiff_encode_none_plan()
    assert pb.strip_rows(100, 500, 16, 0) == 65 and p.per_pass == 1375
    assert p.per_pass < pz.per_pass == pb.tiff_encode_per_pass(100, 500, 16, 8, 0) < pn.per_pass == pb.tiff_encode_per_pass(100, 500, 16, 1, 0)
    assert [q.params["compression"] for q in (p, pz, pn)] == ["lzw", "deflate", "none"]
    # the DEFLATE pass of the Deflate plan: two strings a file, so other counts in the two passes
    assert [(b - a) * 2 for a, b in pz.passes] == [2 * pz.per_pass, 4]
    assert pb.png_encode_plan(16).per_pass == 2049 and pb.png_encode_plan(8).per_pass == 4092
    assert pb.png_encode_plan(16).rows == pb.png_encode_plan(8).rows and pb.png_encode_plan(16).cols == pb.png_encode_plan(8).cols


@pytest.mark.parametrize("make", (pb.jls_decode_rasters_plan, pb.jls_decode_files_plan, pb.tiff_read_rasters_plan, pb.tiff_read_files_plan),
                         ids=lambda f: f.__name__)
def test_decoder_plans_are_cut_by_the_rule_they_name(make):
    p = make()
    files = pb.batch_of(p)[0]
    c0, c1 = p.passes[0]
    first_bytes = sum(len(f) for f in files[c0:c1])
    limit = pb.JLS_PASS_BYTES // 4 if "jpegls" in p.entry else pb.TIFF_PASS_BYTES
    budget = pb.JLS_PASS_BYTES if "jpegls" in p.entry else pb.TIFF_PASS_BYTES
    print(p.describe(), "file bytes of the first pass", first_bytes, "of", limit, "raster bytes", (c1 - c0) * p.raster_bytes, "of", budget)
    assert p.why == [p.params["rule"], "end"]
    if p.params["rule"] == "rasters":
        assert 2 * first_bytes < limit                                              # well below the byte limit
        assert (c1 - c0) * p.raster_bytes <= budget < (c1 + 1 - c0) * p.raster_bytes
    else:
        assert first_bytes <= limit < first_bytes + len(files[c1])                  # h_offsets[c1 + 1] - h_offsets[c0] crosses it
        assert (c1 + 1 - c0) * p.raster_bytes < budget                              # while the rasters do not
    if "tiff" in p.entry and p.params["rule"] == "rasters":
        # the files of each pass that reach the device: both byte orders and more than one coder, and another mix in the short pass than in
        # the full one, so the strip partition (part[0 .. 2], strips[k].file) differs between the passes
        table = pb.batch_of(p)[1]
        mixes = []
        for a, b in p.passes:
            heads = [tm.parse(table[k][0]) for k in {p.key(i) for i in range(a, b)} if table[k][2] != pb.E_TIFF]
            mixes.append(sorted((d["compression"], d["big"]) for d in heads))
            assert {big for _, big in mixes[-1]} == {False, True} and {c for c, _ in mixes[-1]} == {1, 5, 8}, (a, b)
        assert mixes[0] != mixes[1]


@pytest.mark.parametrize("make", pb.REFUSED_PASS_PLANS, ids=lambda f: f.__name__)
def test_a_run_of_refused_files_falls_on_one_pass(make):
    p = make()
    print(p.describe())
    per = p.per_pass
    assert p.passes == [(0, per), (per, 2 * per), (2 * per, p.n)]
    files, table, idx = pb.batch_of(p)
    status = np.array([table[k][2] for k in p.keys()])
    want = {"cct_jpegls_decode_batch": pb.E_JPEGLS, "cct_tiff_read_batch": pb.E_TIFF, "cct_png_read_batch": pb.E_PNG}[p.entry]
    assert (status[per:2 * per] == want).all() and not status[:per].any() and not status[2 * per:].any()
    assert {p.roles.get(i) for i in (0, per - 1, 2 * per, p.n - 1)} == {"planted"}


def test_the_models_refuse_what_the_plans_call_refused():
    for make in pb.BORDER_PLANS:
        p = make()
        files, table, idx = pb.batch_of(p)
        for key, (f, x, status) in table.items():
            assert (x is None) == (status != 0)
            if p.entry == "cct_jpegls_decode_batch":
                try:
                    got = jm.decode_frame(f, p.rows, p.cols, 16)
                    assert status == 0 and np.array_equal(got, x), key
                except jm.JlsError as e:
                    assert status == pb.CODES[e.kind], key
            elif p.entry == "cct_tiff_read_batch":
                got = tm.read(f, p.rows, p.cols, 16)
                assert (pb.CODES[got] == status) if isinstance(got, str) else (status == 0 and np.array_equal(got, x)), key
            else:
                assert pb.png_verdict(f, p.rows, p.cols) == status, key
        roles = {k[0]: s for k, (f, x, s) in table.items()}
        if "host:a" in roles:
            host = {"cct_jpegls_decode_batch": pb.E_JPEGLS, "cct_tiff_read_batch": pb.E_TIFF, "cct_png_read_batch": pb.E_PNG}[p.entry]
            assert roles["host:a"] == roles["host:b"] == host and roles["device:a"] not in (0, host) and roles["device:b"] not in (0, host)


def test_the_png_verdict_is_the_damaged_cases_word():
    """pass_borders.png_verdict gives the PNG plans their codes: held here to every file of png_files.damaged_cases() and to
    the good files of the chunk layer"""
    import png_files as pf
    rows, cols = pf.DAMAGED_SHAPE
    for name, f, x, status in pf.damaged_cases():
        assert pb.png_verdict(f, rows, cols) == status, name
    for name, f, x in pf.chunk_cases():
        assert pb.png_verdict(f, *x.shape) == 0, name
    p = pb.png_read_plan()
    c0 = p.passes[1][0]
    assert [pb.png_file(p, p.key(i))[2] for i in range(c0 - 2, c0 + 2)] == [pb.E_PNG, pb.E_CRC, pb.E_ZLIB, pb.E_PNG]
