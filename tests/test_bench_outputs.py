"""`bench.py --dump-outputs DIR`: the last timed step's VisionFeature / FeatureMatch records as float32 / float64 .npy files
(bench.py: last_step_payloads, dump_outputs), and what a plain run (no --full) does and reports."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from vision_slam_frontend_amd import capi  # noqa: E402


def _payload(feats, pairs):
    """A packed payload in vsf_pack_outputs_dev's layout (header, counts, records)."""
    counts = np.array([len(f) for f in feats] + [len(p) for p in pairs], np.uint32)
    body = b"".join(f.tobytes() for f in feats) + b"".join(p.tobytes() for p in pairs)
    total = 16 + counts.nbytes + len(body)
    hdr = np.array([capi.PAYLOAD_MAGIC, len(feats), len(pairs), total], np.uint32)
    return np.frombuffer(hdr.tobytes() + counts.tobytes() + body, np.uint8)


def _records(rng, n_frames, per_frame):
    feats, pairs = [], []
    for i in range(n_frames):
        f = np.zeros(per_frame + i, capi.VISION_FEATURE_DTYPE)
        f["feature_idx"] = (np.uint64(i) << np.uint64(32)) + np.arange(len(f), dtype=np.uint64)
        f["pixel"] = rng.random((len(f), 2), np.float32) * 640
        f["point3d"] = rng.standard_normal((len(f), 3)).astype(np.float32)
        f["point3d"][::7] = np.nan  # (a point that could not be triangulated)
        feats.append(f)
        m = np.zeros(per_frame // 2 + i, capi.FEATURE_MATCH_DTYPE)
        m["feature_idx_initial"] = np.arange(len(m), dtype=np.uint64) * 3
        m["feature_idx_current"] = np.arange(len(m), dtype=np.uint64) * 5 + (np.uint64(i) << np.uint64(32))
        pairs.append(m)
    return feats, pairs


def _load(d):
    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_dump_writes_every_record_field_exactly(tmp_path):
    feats, pairs = _records(np.random.default_rng(1), 5, 40)
    # two payloads: rank 0's view of a world of two
    shapes = bench.dump_outputs([_payload(feats[:2], pairs[:2]), _payload(feats[2:], pairs[2:])], tmp_path)
    got = _load(tmp_path)
    assert set(got) == set(shapes) == {"features_per_frame", "matches_per_pair", "feature_idx", "feature_pixel",
                                       "feature_point3d", "match_feature_idx"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    f, m = np.concatenate(feats), np.concatenate(pairs)
    assert got["features_per_frame"].tolist() == [len(x) for x in feats]
    assert got["matches_per_pair"].tolist() == [len(x) for x in pairs]
    assert got["feature_idx"].astype(np.uint64).tolist() == f["feature_idx"].tolist()
    assert got["feature_pixel"].tobytes() == f["pixel"].tobytes()
    assert got["feature_point3d"].tobytes() == f["point3d"].tobytes()
    assert got["match_feature_idx"][:, 0].astype(np.uint64).tolist() == m["feature_idx_initial"].tolist()
    assert got["match_feature_idx"][:, 1].astype(np.uint64).tolist() == m["feature_idx_current"].tolist()


def test_dump_over_the_limit_is_a_fixed_sample_within_it(tmp_path):
    feats, pairs = _records(np.random.default_rng(2), 20, 300)
    payload = [_payload(feats, pairs)]
    limit = 64 << 10
    bench.dump_outputs(payload, tmp_path / "a", limit=limit)
    bench.dump_outputs(payload, tmp_path / "b", limit=limit)
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= limit
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a), "the sample is the same every run"
    f, m = np.concatenate(feats), np.concatenate(pairs)
    rows, mrows = a["features_sample_rows"].astype(np.int64), a["matches_sample_rows"].astype(np.int64)
    assert 0 < len(rows) < len(f) and 0 < len(mrows) < len(m)
    assert a["feature_pixel"].tobytes() == f["pixel"][rows].tobytes()
    assert a["match_feature_idx"][:, 1].astype(np.uint64).tolist() == m["feature_idx_current"][mrows].tolist()
    assert a["features_per_frame"].tolist() == [len(x) for x in feats]  # (the counts are whole)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` runs exactly the headline (no leg of --full), reports K steps and
    ms_per_step, and two runs with the same arguments write the same records."""
    args = ["--gpus", "1", "--steps", "4", "--warmup", "1", "--width", "320", "--height", "240", "--batch", "8",
            "--nfeatures", "600"]
    got = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args, "--dump-outputs", str(d)], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 4 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["value"] == pytest.approx(8 * 1e3 / out["ms_per_step"], rel=1e-9)
        for k in ("sustained", "observe_image", "other_configs", "cpu_baseline", "cpu_baseline_native",
                  "stages_ms_per_step_in_line"):
            assert out[k] is None, k
        got.append(_load(d))
    a, b = got
    assert len(a["features_per_frame"]) == 8 and a["features_per_frame"].sum() > 8 * 20
    assert np.isfinite(a["feature_point3d"]).all(axis=1).sum() > 8 * 10  # (triangulated points among them)
    # one temporal pair per frame (window 1); the bench's consecutive frames are different scenes, so few or no records
    assert len(a["matches_per_pair"]) == 8 and a["match_feature_idx"].shape == (a["matches_per_pair"].sum(), 2)
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
