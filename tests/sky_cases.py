"""Skies for the entry-by-entry tests of the sky sampling tables (kernels_sky.hip), shared by test_sky_tables.py (the float64 reference against
itself) and test_gpu_sky_tables.py (the device's read-back, rt_read_sky_tables).

Both scan kernels give thread t of 256 the span [t * per_thread, (t + 1) * per_thread) of the n items, per_thread = ceil(n / 256). The shapes are the
smallest at which each path of that layout runs: 257 (per_thread 2: one thread with a single item behind 128 full spans, 127 empty spans), 256 (the
last size with per_thread 1: the control), 511 / 513 / 515 / 300 / 255 (ragged spans of 2 and 3), 1027 x 515 (5 and 3), and one sky of the size of a
real environment map, 2048 x 1024 (8 and 4). Every case is built from a seed and carries a one-line premise, which `premise` asserts on the
reference (sky_sampling_reference.DeviceTables) -- a case that stops exercising what it is here for fails on the CPU."""
from collections import namedtuple

import numpy as np

import sky_sampling_reference as ref

SUN = 1e5

Case = namedtuple("Case", "name width height premise build check underflows")
CASES = []


def _case(name, width, height, premise, underflows=False):
    def register(pair):
        build, check = pair()
        CASES.append(Case(name, width, height, premise, build, check, underflows))
    return register


def span(i, n):
    """The thread whose span holds item i of n."""
    return i // ref.per_thread(n)


def _random(seed, w, h, high=1.0):
    sky = np.random.default_rng(seed).uniform(0.0, high, (h, w, 4)).astype(np.float32)
    sky[..., 3] = 1.0
    return sky


def _spans_premise(w, h):
    def check(sky, t):
        assert t.w == w and t.h == h and np.all(t.row_total > 0)
    return check


for _seed, (_w, _h, _what) in enumerate([
        (257, 1, "a single row: per_thread 2 in x, thread 128 holds one texel, threads 129..255 none; the marginal has one entry"),
        (1, 257, "a single column: every row's CDF is its forced last entry; the marginal runs per_thread 2 with 127 empty spans"),
        (256, 256, "the control: the last shape at which every thread holds exactly one item"),
        (257, 255, "per_thread 2 in x with a one-item span; 255 rows leave the marginal's last thread empty at per_thread 1"),
        (1027, 515, "per_thread 5 in x (thread 205 holds 2 texels, 50 empty spans) and 3 in y (thread 171 holds 2 rows): no side a multiple of anything"),
]):
    @_case("random_%dx%d" % (_w, _h), _w, _h, "uniform random texels; " + _what)
    def _(seed=_seed, w=_w, h=_h):
        def check(sky, t):
            _spans_premise(w, h)(sky, t)
            assert ref.per_thread(w) == {257: 2, 1: 1, 256: 1, 1027: 5}[w] and ref.per_thread(h) == {1: 1, 257: 2, 256: 1, 255: 1, 515: 3}[h]
            assert len(np.unique(t.lum)) > min(w * h, 200) // 2
        return (lambda: _random(100 + seed, w, h)), check


def _sun_case(name, w, h, sun, premise, extra):
    @_case(name, w, h, premise)
    def _():
        def build():
            return ref.sun_sky(w, h, sun, sun_value=SUN)
        def check(sky, t):
            x, y = sun
            assert np.all(sky[y:y + 2, x:x + 2, 0] == np.float32(SUN)) and (sky[..., 0] == np.float32(SUN)).sum() == 4
            lit = t.lum > 1e4
            ys, xs = np.nonzero(lit)
            assert ys.min() == max(y - 1, 0) and ys.max() == min(y + 2, h - 1) and xs.min() == max(x - 1, 0) and xs.max() == min(x + 2, w - 1)
            assert t.weight[lit].sum() / t.total > 0.2   # the sun carries a large share of the distribution
            extra(x, y)
        return build, check


_sun_case("sun_inside_513x300", 513, 300, (120, 100), "the sun's 2x2 block lies inside thread 40's span in x and inside thread 50's span of the marginal",
          lambda x, y: _assert(span(x, 513) == span(x + 1, 513) == 40 and span(y, 300) == span(y + 1, 300) == 50))
_sun_case("sun_border_x_1027x515", 1027, 515, (429, 100), "the sun's 2x2 block straddles the border between thread 85's and thread 86's span in x",
          lambda x, y: _assert(span(x, 1027) == 85 and span(x + 1, 1027) == 86 and span(y, 515) == span(y + 1, 515)))
_sun_case("sun_border_y_511x257", 511, 257, (200, 119), "the sun's 2x2 block straddles the border between thread 59's and thread 60's span of the marginal",
          lambda x, y: _assert(span(y, 257) == 59 and span(y + 1, 257) == 60 and span(x, 511) == span(x + 1, 511)))
_sun_case("sun_column_0_257x255", 257, 255, (0, 100), "the sun sits in columns 0 and 1: the footprint clamps at x = 0 and the last column stays dim",
          lambda x, y: None)
_sun_case("sun_last_column_513x300", 513, 300, (511, 100), "the sun sits in the last two columns: the footprint clamps at x = W - 1 and column 0 stays dim",
          lambda x, y: None)
_sun_case("sun_row_0_511x257", 511, 257, (200, 0), "the sun sits in rows 0 and 1, the smallest solid angle, where cos t0 - cos t1 cancels",
          lambda x, y: None)
_sun_case("sun_last_row_257x255", 257, 255, (100, 253), "the sun sits in the last two rows, the smallest solid angle at the other pole",
          lambda x, y: None)


def _assert(condition):
    assert condition


BLACK_ROWS = (0, 149, 200, 201, 299)   # the weightless rows of black_rows_513x300


@_case("black_rows_513x300", 513, 300, "weightless rows (three black texel rows each, two at a border): the first, the last, one in the middle, and "
       "rows 200..201 -- the whole span of thread 100 of the marginal")
def _():
    def build():
        sky = _random(11, 513, 300, 2.0)
        sky[0:2, :, :3] = 0.0; sky[298:300, :, :3] = 0.0; sky[148:151, :, :3] = 0.0; sky[199:203, :, :3] = 0.0
        return sky
    def check(sky, t):
        black = np.zeros(300, bool); black[list(BLACK_ROWS)] = True
        assert np.array_equal(t.row_total == 0, black)
        assert ref.per_thread(300) == 2 and span(200, 300) == span(201, 300) == 100 and span(199, 300) == 99 and span(202, 300) == 101
    return build, check


@_case("black_columns_511x257", 511, 257, "black columns at the head (cells 0..5 weightless: entries of 0 in front) and at the tail of every row (cells 501..510 "
       "weightless: the CDF reaches 1 at entry 500, ten entries before the forced 1.0)")
def _():
    def build():
        sky = _random(12, 511, 257, 2.0)
        sky[:, 0:7, :3] = 0.0; sky[:, 500:511, :3] = 0.0
        return sky
    def check(sky, t):
        assert np.all(t.lum[:, :6] == 0) and np.all(t.lum[:, 6:501] > 0) and np.all(t.lum[:, 501:] == 0)
        assert np.all(t.conditional[:, 5] == 0) and np.all(t.conditional[:, 6] > 0)
        assert np.all(t.conditional[:, 499] < 1) and np.all(t.conditional[:, 500:] == 1)
    return build, check


@_case("single_cell_257x255", 257, 255, "one lit texel (100, 127) in a black sky: nine cells carry all the weight, across threads 49 | 50 in x, and "
       "252 rows are weightless")
def _():
    def build():
        sky = np.zeros((255, 257, 4), np.float32); sky[..., 3] = 1.0
        sky[127, 100, :3] = (3.0, 2.0, 1.0)
        return sky
    def check(sky, t):
        ys, xs = np.nonzero(t.lum)
        assert len(ys) == 9 and set(ys) == {126, 127, 128} and set(xs) == {99, 100, 101}
        assert span(99, 257) == 49 and span(100, 257) == 50 and (t.row_total == 0).sum() == 252
    return build, check


@_case("dynamic_range_513x300", 513, 300, "luminances from below 1e-29 to above 1e29 in one sky (one random exponent per 16 x 16 block, random texels inside): "
       "the dim blocks' pdfs underflow float32 and their cells are never picked", underflows=True)
def _():
    def build():
        rng = np.random.default_rng(13)
        exponent = rng.uniform(-30.0, 30.0, (19, 33))
        exponent[3, 4] = -30.0; exponent[9, 20] = 30.0
        e = np.kron(exponent, np.ones((16, 16)))[:300, :513]
        sky = np.ones((300, 513, 4), np.float32)
        sky[..., :3] = (rng.uniform(1.0, 10.0, (300, 513, 3)) * 10.0 ** e[..., None]).astype(np.float32)
        return sky
    def check(sky, t):
        assert np.isfinite(sky).all() and t.lum.min() > 0 and t.lum.min() < 1e-28 and t.lum.max() > 1e30 and np.isfinite(t.total)
        assert (t.cell_pdf == 0).any() and (t.cell_pdf > 0).any()
    return build, check


CONSTANT = (0.25, 0.5, 0.75)


@_case("constant_257x255", 257, 255, "a constant sky: every conditional entry is (x + 1) / W and the marginal is (1 - cos(pi (y + 1) / H)) / 2")
def _():
    def build():
        sky = np.ones((255, 257, 4), np.float32); sky[..., :3] = CONSTANT
        return sky
    def check(sky, t):
        assert len(np.unique(t.lum)) == 1 and t.lum[0, 0] > 0
    return build, check


# (the last case: test_gpu_sky_tables.py goes on with its sky loaded)
@_case("real_size_2048x1024", 2048, 1024, "the size of a real environment map (per_thread 8 and 4): random texels and a 2x2 sun of 1e5 that straddles "
       "threads 85 | 86 in x and threads 74 | 75 of the marginal")
def _():
    x, y = 687, 299
    def build():
        sky = _random(7, 2048, 1024)
        sky[y:y + 2, x:x + 2, :3] = np.float32(SUN)
        return sky
    def check(sky, t):
        assert ref.per_thread(2048) == 8 and ref.per_thread(1024) == 4
        assert span(x, 2048) == 85 and span(x + 1, 2048) == 86 and span(y, 1024) == 74 and span(y + 1, 1024) == 75
        assert (t.lum > 1e4).sum() == 16 and np.all(t.row_total > 0)
    return build, check


BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
