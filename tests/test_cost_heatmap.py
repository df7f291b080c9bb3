"""display.cost_heatmap (CPU): the colour ramp of the traversal-cost view, its scaling and its edge cases."""
import numpy as np
import pytest

from tinsel_amd.display import COST_CHANNELS, cost_heatmap, cost_mean


def _map(values, channel=1):
    m = np.zeros((1, len(values), 4), np.uint32)
    m[0, :, channel] = values
    return m


def test_ramp_end_points_and_interior():
    img = cost_heatmap(_map([0, 300, 600, 900, 150, 450, 750]), "nodes")
    assert img.shape == (1, 7, 4) and img.dtype == np.float32
    want = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (0.5, 0, 0), (1, 0.5, 0), (1, 1, 0.5)]
    np.testing.assert_allclose(img[0, :, :3], np.array(want), atol=1e-6)
    assert (img[..., 3] == 1.0).all()


def test_channel_by_index_or_name():
    m = np.arange(2*3*4, dtype=np.uint32).reshape(2, 3, 4)
    for c, name in enumerate(COST_CHANNELS):
        assert np.array_equal(cost_heatmap(m, c), cost_heatmap(m, name))
        assert np.array_equal(cost_mean(m, name, 2), m[..., c]/2.0)
    with pytest.raises(ValueError):
        cost_heatmap(m, "fetches")
    with pytest.raises(ValueError):
        cost_heatmap(m, 4)
    with pytest.raises(ValueError):
        cost_heatmap(m[..., :3], 0)


def test_vmax_scales_and_clamps():
    m = _map([0, 40, 80, 120], channel=0)
    np.testing.assert_allclose(cost_heatmap(m, "rays", vmax=240)[0, :, :3], [(0, 0, 0), (0.5, 0, 0), (1, 0, 0), (1, 0.5, 0)], atol=1e-6)
    np.testing.assert_allclose(cost_heatmap(m, "rays", vmax=60)[0, :, :3], [(0, 0, 0), (1, 1, 0), (1, 1, 1), (1, 1, 1)], atol=1e-6)
    # the default is the frame's largest mean, whatever the sample count
    assert np.array_equal(cost_heatmap(m, "rays"), cost_heatmap(m, "rays", vmax=120))
    assert np.array_equal(cost_heatmap(m, "rays", samples=4), cost_heatmap(m, "rays", vmax=30, samples=4))
    assert np.array_equal(cost_heatmap(m, "rays", vmax=240), cost_heatmap(m*4, "rays", vmax=240, samples=4))


def test_zero_samples_and_empty_frames_are_black():
    m = _map([5, 10, 15])
    for img in (cost_heatmap(m, "nodes", samples=0), cost_heatmap(np.zeros_like(m), "nodes"), cost_heatmap(m, "nodes", vmax=0)):
        assert not img[..., :3].any() and (img[..., 3] == 1.0).all()
    assert not cost_mean(m, "nodes", 0).any()


def test_write_png_accepts_it(tmp_path):
    from tinsel_amd.display import write_png
    m = _map(np.arange(0, 64, dtype=np.uint32)*7)
    write_png(str(tmp_path / "h.png"), cost_heatmap(m, "nodes"))
    assert (tmp_path / "h.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
