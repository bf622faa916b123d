"""Build and drive the reference-derived oracle binaries (TEST INFRASTRUCTURE ONLY).

For a compiled circuit (circom_amd.compiler.Compiled) this module
  * emits the reference-style <name>.cpp (emit_ref_cpp.py) + copies the .dat next to it under
    oracle/_ref/<prime>/, and compiles `<name>` (the reference's main.cpp CLI: `./name in.json out.wtns`)
    and `<name>_loop` (oracle/ref_loop.cpp) with oracle/Makefile — only possible where the reference tree
    is present; the GPU box uses the prebuilt binaries that travel inside oracle/_ref/,
  * runs them to produce .wtns files / timings.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
REF_ROOT = Path(os.environ.get("CIRCOM_REF", "/root/reference"))


def ref_dir(prime: str) -> Path:
    return ROOT / "_ref" / prime


def binaries(prime: str, name: str):
    d = ref_dir(prime)
    return d / name, d / (name + "_loop")


def build_circuit(cp, force=False, later=None):
    """cp: Compiled.  Returns (cli_binary, loop_binary) or raises if it cannot be built.
    later: a list - the compilation is not run here but appended to it as a callable (build_default_circuits runs those of
    all its circuits side by side: each is minutes of ONE g++ process)."""
    from . import emit_ref_cpp
    from circom_amd.hip_elements.writers import hashmap_size
    prime = cp.flat.prime
    d = ref_dir(prime)
    cli, loop = binaries(prime, cp.name)
    names = d / (cp.name + ".names")
    # the binaries are cached by circuit NAME; the fingerprint (witness code + tables) catches a circuit that changed
    # under the same name, so that a stale reference binary is never compared against
    import hashlib
    h = hashlib.sha256(open(cp.dat_path, "rb").read())          # numbering, hash map, witness list, constants
    for k in sorted(cp.flat.code):                                # the flat witness code (independent of the lowering)
        h.update(k.encode() + bytes(memoryview(cp.flat.code[k])))
    for f in getattr(cp.flat, "functions", ()) or ():           # function bytecode (rewritten by the optimiser), log strings, io map
        h.update(repr(sorted((k, (v.tobytes() if hasattr(v, "tobytes") else repr(v))) for k, v in f.items() if k != "consts")).encode())
    h.update(repr(list(getattr(cp.flat, "log_strings", ()))).encode())
    h.update(repr(getattr(cp.flat, "io_map", ())).encode())
    h.update(open(Path(__file__).resolve().parent / "emit_ref_cpp.py", "rb").read())   # the emitter itself
    h.update(b"CIRCUIT_OPT=-O3")                                  # (oracle/Makefile: binaries built at -O1 in earlier rounds are stale)
    fp = h.hexdigest()
    fp_file = d / (cp.name + ".fp")
    fresh = fp_file.exists() and fp_file.read_text().strip() == fp
    if cli.exists() and loop.exists() and names.exists() and fresh and not force:
        return cli, loop
    if not REF_ROOT.exists():
        raise RuntimeError("oracle/_ref/%s/%s is not prebuilt for this circuit and the reference tree is absent"
                           % (prime, cp.name))
    d.mkdir(parents=True, exist_ok=True)
    emit_ref_cpp.emit(cp.flat, d / (cp.name + ".cpp"), hashmap_size(len(cp.flat.inputs)))
    shutil.copyfile(cp.dat_path, d / (cp.name + ".dat"))
    shutil.copyfile(cp.dat_path, d / (cp.name + "_loop.dat"))
    names.write_text("".join("%s %d\n" % (n, sz) for n, _, sz in cp.flat.inputs))
    name = cp.name

    def compile_():
        for target in ("circuit", "loop"):
            subprocess.run(["make", "-C", str(ROOT), target, "PRIME=" + prime, "NAME=" + name, "REF=" + str(REF_ROOT)],
                           check=True, capture_output=True)
        fp_file.write_text(fp + "\n")
    if later is None:
        compile_()
    else:
        later.append((prime, compile_))
    return cli, loop


def build_cli_with_witness_list(cp, witness2signal, name: str):
    """The reference CLI for the circuit of `cp` with a SIMPLIFIED witness (--O1): `get_size_of_witness()` returns the length of
    the list and the `.dat` carries it (c_code_generator.rs:818-865 writes witness2signal there; calcwit.hpp:54-56 reads the
    witness through it).  Returns the binary; built under oracle/_ref/<prime>/<name>."""
    from . import emit_ref_cpp
    from circom_amd.hip_elements.writers import hashmap_size, write_dat
    if not REF_ROOT.exists():
        raise RuntimeError("the reference tree is absent")
    prime = cp.flat.prime
    d = ref_dir(prime)
    d.mkdir(parents=True, exist_ok=True)
    emit_ref_cpp.emit(cp.flat, d / (name + ".cpp"), hashmap_size(len(cp.flat.inputs)), n_witness=len(witness2signal))
    write_dat(d / (name + ".dat"), cp.flat, witness2signal=witness2signal)
    subprocess.run(["make", "-C", str(ROOT), "circuit", "PRIME=" + prime, "NAME=" + name, "REF=" + str(REF_ROOT)],
                   check=True, capture_output=True)
    return d / name


def run_cli(cp, input_json: str, out_wtns: Path):
    """The reference CLI exactly as a user runs it (main.cpp:336-373)."""
    cli, _ = binaries(cp.flat.prime, cp.name)
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        f.write(input_json)
        p = f.name
    try:
        r = subprocess.run([str(cli), p, str(out_wtns)], capture_output=True, text=True)
    finally:
        os.unlink(p)
    return r


def run_loop(cp, inputs_bytes: bytes, n: int, reps: int = 1, wtns_prefix: str = "", stride: int = 1, procs: int = 1):
    """inputs_bytes: [n][n_inputs][32].  Returns the parsed JSON of each process."""
    prime = cp.flat.prime
    _, loop = binaries(prime, cp.name)
    d = ref_dir(prime)
    with tempfile.TemporaryDirectory() as td:
        per = (n + procs - 1) // procs
        n_in = cp.flat.n_main_inputs
        ps = []
        for k in range(procs):
            lo, hi = k * per, min(n, (k + 1) * per)
            if lo >= hi:
                break
            fn = os.path.join(td, "in%d.bin" % k)
            with open(fn, "wb") as f:
                f.write(inputs_bytes[lo * n_in * 32:hi * n_in * 32])
            cmd = [str(loop), str(d / (cp.name + "_loop.dat")), fn, str(d / (cp.name + ".names")), str(hi - lo), str(reps)]
            if wtns_prefix:
                cmd += [wtns_prefix if procs == 1 else wtns_prefix + "p%d_" % k, str(stride)]
            ps.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        outs = []
        for p in ps:
            o, e = p.communicate()
            if p.returncode != 0:
                raise RuntimeError("ref_loop failed (rc=%d): %s" % (p.returncode, e[-500:]))
            outs.append(json.loads(o.strip().splitlines()[-1]))
    return outs


def host_cores():
    """Cores this process may actually use: the scheduler affinity mask, cut by the cgroup CPU quota when one is set
    (a container that shows 256 CPUs in os.cpu_count() may be limited to ~10 of them by /sys/fs/cgroup/cpu.max).
    Returns (usable, affinity, quota or None)."""
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                if q > 0:
                    quota = q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().split()[0])
            break
        except (OSError, ValueError, IndexError):
            continue
    usable = aff if quota is None else max(1, min(aff, int(quota + 0.5)))
    return usable, aff, quota


def time_reference(cp, workload: str, seconds_budget: float = 15.0):
    """cpu_baseline for bench.py: reference runtime + reference generic (no-asm, GMP) field library on the host
    cores this process can really use (host_cores()), bounded sample.  Two legs:
      (ii) compute-only in-process loop (`run(ctx)` on pre-parsed inputs), one process per usable core -> `value`;
      (i)  end to end as the reference is used: `./<name> input.json out.wtns`, one process per input -> `end_to_end`."""
    import numpy as np
    cli, loop = binaries(cp.flat.prime, cp.name)
    if not (loop.exists()):
        build_circuit(cp)
    cores, affinity, quota = host_cores()
    q = cp.flat.fp.q
    n_in = cp.flat.n_main_inputs
    rng = np.random.default_rng(1)
    def gen(n):
        if workload.startswith("sha256"):
            arr = np.zeros((n, n_in, 32), dtype=np.uint8)
            arr[:, :, 0] = rng.integers(0, 2, size=(n, n_in), dtype=np.uint8)
            return arr.tobytes()
        if workload.startswith("semaphore"):
            # random inputs would trip the circuit's `===` (the reference aborts): valid signatures, tiled
            import random
            from circom_amd.circuits import eddsa_host as H
            r = random.Random(1)
            pool = [b"".join(v.to_bytes(32, "little") for v in H.semaphore_inputs(q, int(workload[9:].rstrip("p") or 20), r)[0])
                    for _ in range(min(n, 16))]
            return b"".join(pool[i % len(pool)] for i in range(n))
        if workload.startswith("ecdsa"):
            # valid secp256k1 signatures (anything else trips the verifier's range checks: the reference aborts), a pool tiled
            import random
            from circom_amd.circuits import secp256k1 as S
            r = random.Random(1)
            pool = [b"".join(int(v).to_bytes(32, "little") for v in S.sign(S.SECP256K1, 64, 4, r)) for _ in range(min(n, 8))]
            return b"".join(pool[i % len(pool)] for i in range(n))
        if workload.startswith("bigmultmodp"):
            # limbs of a, b < p (random field elements would trip the circuit's range checks: the reference aborts)
            import random
            nb, k = ([int(x) for x in workload.split("_")[1:3]] if "_" in workload else (32, 3))
            r = random.Random(1)
            out = []
            for _ in range(n):
                p_ = r.randrange(1 << (nb * k - 1), 1 << (nb * k))
                for x in (r.randrange(p_), r.randrange(p_), p_):
                    out.extend(((x >> (nb * i)) & ((1 << nb) - 1)).to_bytes(32, "little") for i in range(k))
            return b"".join(out)
        vals = [int.from_bytes(rng.bytes(32), "little") % q for _ in range(n * n_in)]
        return b"".join(v.to_bytes(32, "little") for v in vals)
    # calibrate on one core, then a short pilot on all usable cores, and size the sample from the loaded rate
    n0 = 2
    t = run_loop(cp, gen(n0), n0, 1)[0]
    per = t["seconds"] / n0
    n1 = max(2, min(20000, int(2.0 / max(per, 1e-6))))          # ~2 s on ONE core
    single = run_loop(cp, gen(n1), n1, 1)[0]["witnesses_per_s"]
    n_pilot = max(1, min(5000, int(0.2 / max(per, 1e-6))))
    pilot = run_loop(cp, gen(n_pilot) * cores, n_pilot * cores, 1, procs=cores)
    per_loaded = max(o["seconds"] for o in pilot) / n_pilot       # compute seconds per instance per core, all cores busy
    n_per_core = max(1, min(20000, int(seconds_budget * 0.5 / max(per_loaded, 1e-6))))
    n = n_per_core * cores
    t0 = time.perf_counter()
    outs = run_loop(cp, gen(n_per_core) * cores, n, 1, procs=cores)
    wall = time.perf_counter() - t0
    agg = sum(o["witnesses_per_s"] for o in outs)
    res = {"value": agg, "unit": "witnesses/s", "cores": cores, "kind": "reference",
           "per_core": agg / cores, "single_core_alone": single,
           "cores_detail": {"os_cpu_count": os.cpu_count(), "sched_affinity": affinity, "cgroup_quota": quota},
           "sample": "%d instances (%d per core x %d cores) of %s through the reference C++ runtime "
                     "(common/calcwit.cpp + generic/fr.cpp --no_asm GMP build), compute-only in-process loop, "
                     "wall %.1f s" % (n, n_per_core, cores, workload, wall),
           # the field library and the runtime are built at -O3 as the reference's makefile does (c_elements/generic/makefile:2);
           # the circuit's own <name>.cpp - a straight line of calls into them, 10 MB of source per SHA-256 block pair - at -O3 as
           # well (oracle/Makefile CIRCUIT_OPT = c_elements/generic/makefile:2; round 4 built it at -O1)
           "circuit_opt": "fr.cpp / calcwit.cpp / main.cpp / <name>.cpp all -O3 (oracle/Makefile, as c_elements/generic/makefile)"}
    # (i) end to end: JSON parse + process start + .dat load + compute + .wtns write, `cores` processes at a time
    try:
        res["end_to_end"] = _time_cli(cp, gen, cores, min(8.0, seconds_budget * 0.5))
    except Exception as e:      # a report, never a reason to fail
        res["end_to_end"] = {"value": None, "error": str(e)[:200]}
    return res


def _time_cli(cp, gen, cores, budget):
    cli, _ = binaries(cp.flat.prime, cp.name)
    n_in = cp.flat.n_main_inputs
    raw = gen(4)
    with tempfile.TemporaryDirectory() as td:
        files = []
        for i in range(4):
            vals = [int.from_bytes(raw[(i * n_in + k) * 32:(i * n_in + k + 1) * 32], "little") for k in range(n_in)]
            obj, pos = {}, 0
            for name, _, size in cp.flat.inputs:
                dims = cp.flat.input_dims.get(name) or []
                obj[name] = str(vals[pos]) if not dims else [str(v) for v in vals[pos:pos + size]]
                pos += size
            fn = os.path.join(td, "in%d.json" % i)
            json.dump(obj, open(fn, "w"))
            files.append(fn)
        t0 = time.perf_counter()
        r = subprocess.run([str(cli), files[0], os.path.join(td, "w0.wtns")], capture_output=True)
        one = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("reference CLI failed: %s" % r.stderr[-200:])
        rounds = max(1, int(budget / max(one, 1e-3) / 2))
        t0 = time.perf_counter()
        done = 0
        for _ in range(rounds):
            ps = [subprocess.Popen([str(cli), files[k % 4], os.path.join(td, "w%d.wtns" % k)], stdout=subprocess.DEVNULL,
                                   stderr=subprocess.DEVNULL) for k in range(cores)]
            for p_ in ps:
                p_.wait()
                done += 1
        wall = time.perf_counter() - t0
    return {"value": done / wall, "unit": "witnesses/s", "cores": cores, "seconds_per_witness_one_process": one,
            "sample": "%d runs of `./%s input.json out.wtns` (%d at a time)" % (done, cp.name, cores)}


def _flat_only(prog, d, name):
    """what build_circuit needs of a compiled circuit - the flat program and its .dat - without lowering it (minutes for the
    ECDSA verifier)"""
    from types import SimpleNamespace
    from circom_amd.frontend.flatten import flatten
    from circom_amd.hip_elements import writers
    fc = flatten(prog)
    dat = os.path.join(d, name + ".dat")
    writers.write_dat(dat, fc)
    return SimpleNamespace(name=name, flat=fc, dat_path=dat)


def build_default_circuits():
    """Called from __graft_entry__.build(): prebuild the oracle binaries the GPU-side tests/bench use."""
    import hashlib
    import tempfile as _t
    import bench
    # Tracing the nine circuits only to find their binaries current is two minutes: a stamp keyed by everything that shapes them
    # (the sources bench.artefact_fingerprint covers + this directory's emitter / drivers / recipe) short-cuts a repeated build()
    h = hashlib.sha256(bench.artefact_fingerprint().encode())
    for f in sorted(list(ROOT.glob("*.py")) + list(ROOT.glob("*.cpp")) + [ROOT / "Makefile"]):
        h.update(f.name.encode() + open(f, "rb").read())
    stamp = ref_dir("bn128").parent / ".default_circuits"
    wanted = [binaries("bn128", n) for n in ("multiplier2", "poseidon2", "sha256_512", "semaphore20", "semaphore20p", "semaphore20w",
                                             "sha256_2048")] + [binaries("bls12381", n) for n in ("bigmultmodp", "ecdsa_verify")]
    if stamp.exists() and stamp.read_text().strip() == h.hexdigest() and all(c.exists() and l.exists() for c, l in wanted) \
            and (ref_dir("goldilocks") / "poseidon2").exists():
        return
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    from circom_amd.circuits.basic import Multiplier2
    from circom_amd.circuits.poseidon import Poseidon
    d = _t.mkdtemp(prefix="cw_refbuild_")
    jobs = []               # the circuits' compilations: emitted one after the other (Python), compiled side by side (g++)
    from circom_amd.circuits.sha256 import Sha256
    from circom_amd.circuits.eddsa import SemaphoreStyle
    from circom_amd.circuits.bigint import BigMultModP
    for name, prog in (("multiplier2", Program(Multiplier2())), ("poseidon2", Program(Poseidon(2))),
                       ("bigmultmodp", Program(BigMultModP(32, 3), prime="bls12381")),
                       ("sha256_512", Program(Sha256(512))), ("semaphore20", Program(SemaphoreStyle(20))),
                       ("semaphore20p", Program(SemaphoreStyle(20, True))), ("semaphore20w", Program(SemaphoreStyle(20, "window"))),
                       ("sha256_2048", Program(Sha256(2048)))):
        # (only the flat circuit and the .dat are needed here: one strand variant, no emitted code)
        cp = compile_program(prog, d, name, sym=False, strands=(1,), jit=False, fpjit=False)
        build_circuit(cp, later=jobs)
    # BASELINE config 5's verifier (2.47 M signals: half a minute of tracing, minutes of g++): parity + CPU baseline of its bench line
    # (only the flat program and its .dat: build_circuit compares fingerprints and returns when the binary is current)
    build_circuit(_flat_only(bench.make_program("ecdsa_verify"), d, "ecdsa_verify"), later=jobs)
    if jobs:
        import concurrent.futures as cf
        # what the circuits of one prime share (the field library and runtime of `ref`, the renamed main.cpp, the loop driver)
        # first, once: no two makes write one file
        for prime in sorted({p_ for p_, _ in jobs}):
            subprocess.run(["make", "-C", str(ROOT), "ref", "_ref/%s/main_lib.o" % prime, "_ref/%s/ref_loop.o" % prime, "PRIME=" + prime,
                            "REF=" + str(REF_ROOT)], check=True, capture_output=True)
        # at most four at a time: g++ -O3 on the 10 MB source of a million-signal circuit holds gigabytes
        with cf.ThreadPoolExecutor(max_workers=max(1, min(len(jobs), host_cores()[0], 4))) as ex:
            for f_ in [ex.submit(j_) for _, j_ in jobs]:
                f_.result()
    # the reference's 64-bit runtime for `bench.py --workload poseidon2_goldilocks` (parity + CPU baseline of that line)
    from circom_amd.frontend.flatten import flatten
    if not (ref_dir("goldilocks") / "poseidon2").exists():
        build_circuit64(flatten(Program(Poseidon(2), prime="goldilocks")), "poseidon2")
    stamp.write_text(h.hexdigest() + "\n")


# ---- the 64-bit runtime (`--prime goldilocks`): oracle side only -------------------------------------------------------
# The device path refuses this prime (DESIGN 9 / NOTES: its "q is large" shortcuts); the oracle is pinned against the
# reference's own 64-bit runtime here so that a later round only has device work left.
def write_dat64(path, fc):
    """the product's own writer (hip_elements/lower64.py): the file the reference's 64-bit runtime loads"""
    from circom_amd.hip_elements.lower64 import write_dat64 as w
    return w(path, fc)


def build_circuit64(fc, name: str):
    """reference CLI of a goldilocks circuit: oracle/_ref/goldilocks/<name> (emit_ref_cpp in its 64-bit mode + oracle/Makefile
    circuit64).  Needs the reference tree."""
    from . import emit_ref_cpp
    assert fc.prime == "goldilocks"
    if not REF_ROOT.exists():
        raise RuntimeError("the reference tree is absent")
    d = ref_dir("goldilocks")
    d.mkdir(parents=True, exist_ok=True)
    size = write_dat64(d / (name + ".dat"), fc)
    emit_ref_cpp.emit(fc, d / (name + ".cpp"), size)
    subprocess.run(["make", "-C", str(ROOT), "circuit64", "NAME=" + name, "REF=" + str(REF_ROOT)], check=True, capture_output=True)
    return d / name


def run_cli64(cli: Path, input_json: str, out_wtns: Path):
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        f.write(input_json)
        p = f.name
    try:
        return subprocess.run([str(cli), p, str(out_wtns)], capture_output=True, text=True)
    finally:
        os.unlink(p)


def time_fp_mul(prime: str = "bn128", seconds_budget: float = 4.0):
    """The "Fp mul/s" half of the metric on the host: the reference's own `Fr_mul` (generic/fr.cpp:559-637,
    long Montgomery x long Montgomery -> Fr_rawMMul :110-164) in a dependent chain, one chain per usable core (ctypes releases
    the GIL for the length of the call), through oracle/_ref/<prime>/libfr_shim.so (fr_shim.cpp ofr_mul_chain).  The chain's end
    value is checked against Python integers.  Returns a dict for bench.py's cpu_baseline (never raises past the caller's try)."""
    import threading
    from .ref_shim import RefFr
    so = ref_dir(prime) / "libfr_shim.so"
    fr = RefFr(so)
    q = fr.q
    a, b = 0x1234567890ABCDEF1234567890ABCDEF % q, (q - 0xFEDCBA987654321) % q
    cores, affinity, quota = host_cores()
    n0 = 1 << 20
    t0 = time.perf_counter()
    got = fr.mul_chain(a, b, n0)
    dt = max(time.perf_counter() - t0, 1e-6)
    assert got == a * pow(b, n0, q) % q, "Fr_mul chain differs from Python integers"     # (the shim converts at its boundary)
    single = n0 / dt
    n = max(n0, int(single * seconds_budget * 0.8))
    secs = [0.0] * cores

    def work(k):
        t1 = time.perf_counter()
        fr.mul_chain(a + k, b, n)
        secs[k] = time.perf_counter() - t1
    th = [threading.Thread(target=work, args=(k,)) for k in range(cores)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    wall = time.perf_counter() - t0
    agg = sum(n / s for s in secs if s > 0)
    return {"value": agg, "unit": "Fp-mul/s", "cores": cores, "per_core": agg / cores, "single_core_alone": single, "prime": prime,
            "kind": "reference",
            "sample": "%d dependent Fr_mul (Montgomery x Montgomery, generic/fr.cpp --no_asm build) per core x %d cores, wall %.1f s; "
                      "chain end value checked against Python integers" % (n, cores, wall)}
