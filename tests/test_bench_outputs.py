"""Host-side checks of two things bench.py does around its timed steps: the files of `--dump-outputs` (dump_outputs) and the
artefact cache when this user may only read it (get_compiled)."""
import gzip
import os
import shutil
import stat
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


class _Circ:
    def __init__(self, n_witness, n_public):
        self.n_witness, self.n_public = n_witness, n_public


class _Batch:
    """what dump_outputs asks of a batch: its size, the status words and one instance's witness image"""

    def __init__(self, n, n_witness):
        self.n, self.n_witness = n, n_witness

    def status(self):
        return (np.arange(self.n, dtype=np.uint32) % 7 == 3).astype(np.uint32) * 5

    def witness_bytes(self, i):
        v = (np.arange(self.n_witness, dtype=np.uint64) * 2654435761 + i) % (1 << 32)
        img = np.zeros((self.n_witness, 8), dtype="<u4")
        img[:, 0] = v
        img[:, 7] = i
        return img.tobytes()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("B,n_wit,n_pub", [(300, 50, 3), (3 << 20, 100_000, 0), (4096, 40_000, 256)])
def test_dump_outputs_shapes_bound_and_seeded_sample(tmp_path, B, n_wit, n_pub):
    import torch
    import bench
    circ, batch = _Circ(n_wit, n_pub), _Batch(B, n_wit)
    pub = None
    if n_pub:
        g = torch.Generator().manual_seed(3)
        pub = torch.randint(0, 256, (B, n_pub, 32), dtype=torch.uint8, generator=g)
    info = bench.dump_outputs(str(tmp_path / "a"), batch, circ, pub)
    bench.dump_outputs(str(tmp_path / "b"), batch, circ, pub)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(info["files"]) == sorted(b)
    total = 0
    for k in a:
        assert a[k].dtype == np.float64
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), "two dumps of the same outputs differ in " + k
        total += os.path.getsize(tmp_path / "a" / (k + ".npy"))
    assert total <= 64_000_000 and info["bytes"] <= total
    # the status words, where they belong
    si = a["status_instances"].astype(np.int64)
    assert len(si) == min(B, 1 << 20) and (np.diff(si) > 0).all() and si[-1] < B
    assert (a["status"] == batch.status()[si]).all()
    # witness wires: eight 32-bit limbs each, of the first and the last instance
    wi = a["witness_sample_wires"].astype(np.int64)
    assert a["witness_sample"].shape == (len({0, B - 1}), len(wi), 8) and len(wi) == min(n_wit, 32768)
    assert (a["witness_sample"][-1, :, 7] == B - 1).all()
    assert (a["witness_sample"][0, :, 0] == (wi.astype(np.uint64) * 2654435761) % (1 << 32)).all()
    if n_pub:
        pi = a["public_signals_instances"].astype(np.int64)
        assert a["public_signals"].shape == (len(pi), n_pub, 8) and len(pi) == min(B, (16 << 20) // (64 * n_pub))
        want = pub.numpy()[pi].view("<u4").astype(np.float64).reshape(len(pi), n_pub, 8)
        assert (a["public_signals"] == want).all()
    else:
        assert "public_signals" not in a


def _read_only(d):
    for r, ds, fs in os.walk(d):
        for n in fs:
            os.chmod(os.path.join(r, n), stat.S_IRUSR | stat.S_IRGRP | stat.S_IROTH)
        os.chmod(r, stat.S_IRUSR | stat.S_IXUSR)


def _writable_again(d):
    for r, ds, fs in os.walk(d):
        os.chmod(r, stat.S_IRWXU)


@pytest.mark.slow
def test_get_compiled_with_a_cache_this_user_may_only_read(tmp_path, monkeypatch):
    """an entry of a read-only cache is used where it lies, what must be written (lock, unpacked files, a lowering that is
    not there) goes to the user's own entry under the temporary directory, and the cache itself is left untouched"""
    if os.geteuid() == 0:
        pytest.skip("root may write into a read-only directory: nothing to test as root")
    import bench
    name, B = "poseidon2", 64
    empty, shared, t1, t2 = (tmp_path / n for n in ("empty", "shared", "t1", "t2"))
    for d in (empty, shared, t1, t2):
        d.mkdir()
    try:
        # no entry, and no right to make one: lowered into the own entry, found there the next time
        _read_only(empty)
        monkeypatch.setattr(tempfile, "tempdir", str(t1))
        cp, _, cached = bench.get_compiled(name, B, str(empty), 0, None)
        assert not cached and cp.tape_path.startswith(str(t1)) and os.path.exists(cp.tape_path)
        cp2, _, cached = bench.get_compiled(name, B, str(empty), 0, None, flat=False)
        assert cached and cp2.tape_path == cp.tape_path and cp2.flat is None
        assert os.listdir(empty) == []
        # an entry whose tape lies compressed: unpacked into the own entry, the rest read where it lies
        entry = shared / os.path.basename(cp.dir)
        shutil.copytree(cp.dir, entry)
        with open(entry / (name + ".cwt"), "rb") as fi, gzip.open(entry / (name + ".cwt.gz"), "wb") as fo:
            shutil.copyfileobj(fi, fo)
        os.unlink(entry / (name + ".cwt"))
        before = sorted(os.listdir(entry))
        _read_only(shared)
        monkeypatch.setattr(tempfile, "tempdir", str(t2))
        cp3, _, cached = bench.get_compiled(name, B, str(shared), 0, None, flat=False)
        assert cached and cp3.dir == str(entry)
        assert cp3.tape_path.startswith(str(t2)) and open(cp3.tape_path, "rb").read() == open(cp.tape_path, "rb").read()
        assert cp3.dat_path == str(entry / (name + ".dat")) and cp3.r1cs_path == str(entry / (name + ".r1cs"))
        assert sorted(os.listdir(entry)) == before and sorted(os.listdir(shared)) == [entry.name]
        from circom_amd import runtime as rt
        c = rt.Circuit(cp3.tape_path, cp3.dat_path, cp3.r1cs_path)          # (host side: the loader takes the files)
        assert c.n_constraints > 0
        c.close()
        # nowhere to write at all: said so, not a missing file later
        t3 = tmp_path / "t3"
        t3.mkdir()
        _read_only(t3)
        monkeypatch.setattr(tempfile, "tempdir", str(t3))
        with pytest.raises((OSError, RuntimeError)):
            bench.get_compiled(name, B, str(shared), 0, None, flat=False)
    finally:
        for d in (empty, shared, tmp_path / "t3"):
            if d.exists():
                _writable_again(d)
