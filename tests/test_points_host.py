"""The argument checks of the point-table entry points (csrc/points.hip, points_local.hip, kitti_frame.hip, nuscenes_frame.hip)
without a GPU: sizes are refused with -1 and the entry point's own message before anything is launched or dereferenced, and an
empty table is served (0) without a look at any pointer."""
import pytest

from toda_amd import lib as L

FAKE = 4096        # a non-null "pointer" for arguments a refused call must not touch
ZEROS = L.host_f64([0.0] * 64)        # a readable host table: an entry point may read its host arguments before it looks at the device's


# entry point -> its arguments behind (points, n, n_dev, c) for a table pointer p (FAKE or None)
ROW_PASSES = {
    "points_in_boxes": lambda p: (p, 3, 7, 0, p, None),
    "points_sector": lambda p: (-0.5, 1.2, p, None),
    "points_rect": lambda p: (p, p, 0, p, None),
    "points_polar_cell": lambda p: (0.5, p, 2, p, 3, 1e-5, 54.0, p, None),
    "points_polar_select": lambda p: (-0.5, 1.2, 1, 0, 0.0, None, p, None),
    "points_pitch_band": lambda p: (-1.8, -20.0, 0.0, p, 5, p, None),
    "points_rotate_z": lambda p: (0.6, 0.8, p, None),
    "points_world_transform": lambda p: (1, 0, 1, 0.6, 0.8, 1, 1.05, p, None),
    "points_box_steps": lambda p: (p, 3, p, p, None),
    "points_in_pyramids": lambda p: (p, 3, p, p, None),
    "points_fov_flags": lambda p: (p, p, 375, 1242, p, None),
}


def call(name, points, n, c, tail):
    return getattr(L.load(), "toda_" + name)(points, n, None, c, *tail)


def last_error():
    return L.load().toda_last_error().decode()


@pytest.mark.parametrize("name", sorted(ROW_PASSES))
def test_row_passes_refuse_bad_sizes_with_their_own_message(name):
    for n, c in ((-1, 4), (10, 2), (-1, 2)):
        assert call(name, FAKE, n, c, ROW_PASSES[name](FAKE)) == -1
        assert last_error() == name + ": need n >= 0 and at least 3 columns (x, y, z)"


@pytest.mark.parametrize("name", sorted(ROW_PASSES))
def test_row_passes_serve_an_empty_table_without_its_pointers(name):
    for c in (3, 4, 5):
        assert call(name, None, 0, c, ROW_PASSES[name](None)) == 0


@pytest.mark.parametrize("name", sorted(ROW_PASSES))
def test_row_passes_refuse_null_tables(name):
    assert call(name, None, 10, 4, ROW_PASSES[name](None)) == -1 and "null" in last_error()
    assert call(name, None, 10, 4, ROW_PASSES[name](L.hptr(ZEROS))) == -1 and "null" in last_error()    # the table itself


def test_the_sizes_of_a_row_pass_come_before_the_empty_table():
    """sizes first, then n == 0, then pointers: an empty table does not excuse a bad size"""
    lib = L.load()
    assert lib.toda_points_in_boxes(None, 0, None, 4, None, 4097, 7, 0, None, None) == -1 and "k in [0,4096]" in last_error()
    assert lib.toda_points_polar_cell(None, 0, None, 4, 0.5, None, 0, None, 3, 1e-5, 54.0, None, None) == -1 and "1..32 bins" in last_error()
    assert lib.toda_points_polar_select(None, 0, None, 4, -0.5, 1.2, 3, 0, 0.0, None, None, None) == -1 and "yaw_mode 1|2" in last_error()
    assert lib.toda_points_pitch_band(None, 0, None, 4, -1.8, -20.0, 0.0, None, 33, None, None) == -1 and "1..32 bands" in last_error()
    assert lib.toda_points_box_steps(None, 0, None, 4, None, -1, None, None, None) == -1 and "n_steps >= 0" in last_error()
    assert lib.toda_points_in_pyramids(None, 0, None, 4, None, -1, None, None, None) == -1 and "pyramid count >= 0" in last_error()
    assert lib.toda_points_fov_flags(None, 0, None, 4, None, None, 0, 1242, None, None) == -1
    assert last_error() == "points_fov_flags: image size 0 x 1242 is not positive"


def test_range_reductions_have_their_own_size_rules_and_always_a_result():
    lib = L.load()
    big = 1 << 20
    assert lib.toda_points_pitch_range_workspace_bytes() == lib.toda_points_column_range_workspace_bytes() == 256 * 2 * 4
    for n, c in ((-1, 4), (10, 2)):
        assert lib.toda_points_pitch_range(FAKE, n, None, c, FAKE, FAKE, big, None) == -1
        assert last_error() == "points_pitch_range: need n >= 0 and at least 3 columns (x, y, z)"
    for n, c, col in ((-1, 4, 0), (10, 0, 0), (10, 4, 4), (10, 4, -1)):
        assert lib.toda_points_column_range(FAKE, n, None, c, col, FAKE, FAKE, big, None) == -1
        assert last_error() == "points_column_range: need n >= 0 and a column in [0, c)"
    assert lib.toda_points_column_range(FAKE, 10, None, 1, 0, FAKE, FAKE, 2047, None) != 0                # one column is a table here
    assert last_error() == "points_column_range: workspace 2047 < required 2048"
    assert lib.toda_points_pitch_range(FAKE, 10, None, 4, FAKE, FAKE, 2047, None) != 0
    assert last_error() == "points_pitch_range: workspace 2047 < required 2048"
    # n == 0 still writes (+inf, -inf): only the table may be null then
    assert lib.toda_points_pitch_range(None, 0, None, 4, None, None, big, None) == -1 and "null" in last_error()
    assert lib.toda_points_column_range(None, 0, None, 4, 2, None, None, big, None) == -1 and "null" in last_error()


def test_sweeps_merge_and_select_append_have_their_own_size_rules():
    lib = L.load()
    bound = lib.toda_sweeps_merge_max_sweeps()

    def merge(n, s, p, radius=1.0):
        return lib.toda_sweeps_merge(p, n, s, p, p, p, p, p, radius, None, p, p, None)

    assert merge(-1, 1, FAKE) == -1 and last_error() == "sweeps_merge: need n >= 0"
    for s in (0, bound + 1):
        assert merge(8, s, FAKE) == -1
        assert last_error() == "sweeps_merge: %d sweeps, supported are 1 to %d (key frame included)" % (s, bound)
    assert merge(8, 1, FAKE, radius=-1.0) == -1 and last_error() == "sweeps_merge: the ego radius must be a number >= 0"
    assert merge(0, 0, None) == -1 and merge(0, 1, None, radius=float("nan")) == -1                      # sizes come first
    assert merge(0, 1, None) == 0 and merge(0, bound, None) == 0
    assert merge(8, 1, None) == -1 and last_error() == "sweeps_merge: null sweep table"

    def append(n, c, cap, p, ws_bytes=1 << 20):
        return lib.toda_rows_select_append(p, n, None, c, p, 1, 0, p, cap, p, p, ws_bytes, None)

    for n, c, cap in ((-1, 4, 10), (10, 0, 10), (10, 4, -1)):
        assert append(n, c, cap, FAKE) == -1 and last_error() == "rows_select_append: bad sizes"
    assert append(0, 1, 0, None) == 0
    assert append(1000, 4, 10, None, ws_bytes=16) != 0 and "workspace" in last_error()
