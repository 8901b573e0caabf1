"""The decode launch plan (welle.io_amd/csrc/dabphy_fused.hip: fused_plan) case by case, to compare two builds of the library on ONE
platform (the execution model with itself, the device with itself): one small case per branch of the plan, each in a fresh child
process.  Per case: the "decode plan for" lines of stderr (experiments builds, DABPHY_DEBUG), last_decode_plan(), a SHA-256 of the FIBs
and of every sub-channel's decoded rows, and -- on the execution model -- a SHA-256 of the queue-order trace started in front of
dabphy_create, so that the first call's uploads are in it.
Usage: python tools/decode_plan_digest.py <library>"""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: F401,E402
import parity_cases as P  # noqa: E402
from welle_io_amd import capi, synth  # noqa: E402

SWITCHES = ("DABPHY_SP_MAX_CW", "DABPHY_SP2_MIN_CW", "DABPHY_FUSED_MSC", "DABPHY_FUSED_FIC", "DABPHY_TB_SPLIT", "DABPHY_FORCE_DEC_BY_ITEM")
ALL18 = tuple(range(18))


def stream_calls(calls, subs=(3, 10), subs2=None, B=1, max_frames=None, mixed=False, **cfg):
    """calls: frames per call, one entry per dabphy_process; subs2: the list from the second call on"""
    return dict(kind="stream", calls=calls, subs=subs, subs2=subs2, B=B, max_frames=max_frames or max(calls), mixed=mixed, cfg=cfg)


def seam(name, n_cw):
    return dict(kind="seam", seam=name, n_cw=n_cw)


# name: (what runs, environment of the experiments build).  State-parallel cases stay at one ensemble and a few frames (the execution
# model runs those kernels a wavefront at a time)
CASES = {
    "depth_1_rows_324": (stream_calls([1, 1, 1], decode_shape=1), {}),
    "depth_4_rows_144": (stream_calls([4, 4], subs=ALL18, decode_shape=1), {}),
    "depth_16_rows_96": (stream_calls([16], subs=(0, 5, 9), decode_shape=1), {}),
    "decode_shape_1": (stream_calls([2, 2], B=2, decode_shape=1), {}),
    "decode_shape_2": (stream_calls([1, 1], decode_shape=2), {}),
    "decode_shape_3": (stream_calls([1, 1], decode_shape=3), {}),
    "decode_shape_0": (stream_calls([1, 1]), {}),
    "decode_shape_0_sp_max_cw_0": (stream_calls([1, 1]), {"DABPHY_SP_MAX_CW": "0"}),
    "fused_msc_0": (stream_calls([3, 3], subs=(0, 5, 9), B=2, decode_shape=1), {"DABPHY_FUSED_MSC": "0"}),
    "fused_fic_0": (stream_calls([3, 3], subs=(0, 5, 9), B=2, decode_shape=1), {"DABPHY_FUSED_FIC": "0"}),
    "tb_split_1": (stream_calls([3, 3], subs=(0, 5, 9), B=2, decode_shape=1), {"DABPHY_TB_SPLIT": "1"}),
    "force_dec_by_item_1": (stream_calls([3, 3], subs=(0, 5, 9), B=2, decode_shape=1), {"DABPHY_FORCE_DEC_BY_ITEM": "1"}),
    "mixed_ensemble": (stream_calls([4, 4], subs=None, B=2, mixed=True, decode_shape=1), {}),
    "list_changed": (stream_calls([2, 2, 2], subs=(0, 5, 9), subs2=(5, 11, 12, 17), B=2, decode_shape=1), {}),
    "list_changed_state_parallel": (stream_calls([1, 1, 1], subs=(3,), subs2=(3, 10)), {}),
    "fewer_frames": (stream_calls([4, 2, 4], subs=(0, 5, 9), B=2, decode_shape=1), {}),
    "exact_batch_replay": (stream_calls([4, 4], subs=(0, 5, 9), B=2, exact_batch=True, replay=True, decode_shape=1), {}),
    "exact_batch_replay_state_parallel": (stream_calls([4, 4], subs=(5,), exact_batch=True, replay=True, decode_shape=2), {}),
    "seam_viterbi_batch_3": (seam("viterbi_batch", 3), {}),
    "seam_viterbi_batch_1100": (seam("viterbi_batch", 1100), {}),
    "seam_msc_deconvolve_3": (seam("msc_deconvolve", 3), {}),
    "seam_msc_deconvolve_1100": (seam("msc_deconvolve", 1100), {}),
    "seam_fic_decode_3": (seam("fic_decode", 3), {}),
    "seam_fic_decode_1100": (seam("fic_decode", 1100), {}),
}


def make_streams(folder):
    """the one stream (18 sub-channels of 64 kbit/s; 3 dB, -1000 Hz: four frames per call decode its first batch twice in exact batch
    mode) and the mixed ensemble's, as the children load them"""
    x = synth.make_stream(25, snr_db=3, cfo_hz=-1000, delay=150, seed=5)
    np.save(os.path.join(folder, "stream.npy"), np.asarray(x, np.complex64))
    xm = synth.make_stream(11, subchs=P.mixed_subchannels(), snr_db=12, cfo_hz=-55, delay=123, seed=31)
    np.save(os.path.join(folder, "mixed.npy"), np.asarray(xm, np.complex64))


def sha(*arrays):
    s = hashlib.sha256()
    for a in arrays:
        s.update(np.ascontiguousarray(a).tobytes())
    return s.hexdigest()


def run_stream(d, c, folder):
    subchs = P.mixed_subchannels() if c["mixed"] else synth.default_subchannels()
    x = np.load(os.path.join(folder, "mixed.npy" if c["mixed"] else "stream.npy"))
    pick = lambda idx: [(s.subch_id, s.start_cu, s.size_cu, P.dev_prot(d, s)) for s in (subchs if idx is None else [subchs[i] for i in idx])]
    d.stream_upload(np.tile(x, (c["B"], 1)))
    subs = pick(c["subs"])
    d.set_subchannels(subs)
    for k, F in enumerate(c["calls"]):
        if k == 1 and c["subs2"] is not None:
            subs = pick(c["subs2"])
            d.set_subchannels(subs)
        d.process(F)
        print("  call %d: %d frames, plan %s, FIBs %s, MSC %s" % (k, F, d.last_decode_plan(), sha(*d.fibs()), sha(*[d.msc(i)[0] for i in range(len(subs))])))
        if k == 0 and c["cfg"].get("replay"):
            d.reset()                                       # (the batch that acquires is the one decoded twice: once more, as a later call)
    if c["cfg"].get("replay"):
        print("  replayed batches: %d" % d.replayed_batches())


def run_seam(d, c):
    rng = np.random.RandomState(11)
    n = c["n_cw"]
    if c["seam"] == "viterbi_batch":
        out = d.viterbi_batch(rng.randint(-128, 128, (n, 4 * (768 + 6))).astype(np.int8), 768)
    elif c["seam"] == "msc_deconvolve":
        p = d.protection_eep(32, False, 3)
        out = d.msc_deconvolve(p, rng.randint(-128, 128, (n, d.protection_input_bits(p))).astype(np.int8))
    else:
        out = np.concatenate([np.ravel(a) for a in d.fic_decode(rng.randint(-128, 128, ((n + 3) // 4, 9216)).astype(np.int8))[:2]])
    print("  %s of %d code words: %s" % (c["seam"], n, sha(out)))


def child(lib_path, name, folder):
    c, switches = CASES[name]
    for k in SWITCHES:                                      # (tests/conftest.py sets DABPHY_SP_MAX_CW=0 for the GPU-less suite: unset here means unset)
        if k not in switches:
            os.environ.pop(k, None)
    lib = C.CDLL(lib_path)
    emu = hasattr(lib, "hipemu_trace_start")
    if emu:
        lib.hipemu_trace_read.restype = C.c_int64
        lib.hipemu_trace_start()
    cfg = {k: v for k, v in c.get("cfg", {}).items() if k != "replay"}
    cfg.setdefault("exact_batch", False)
    d = capi.DabPhy(lib_path=lib_path, n_ensembles=c.get("B", 1), max_frames=c.get("max_frames", 1), want_constellation=False, want_impulse_response=False, **cfg)
    try:
        run_stream(d, c, folder) if c["kind"] == "stream" else run_seam(d, c)
        if emu:
            n = lib.hipemu_trace_read(None, C.c_int64(0))
            buf = C.create_string_buffer(max(n, 1))
            assert lib.hipemu_trace_read(buf, C.c_int64(n)) == n
            print("  queue order: %d records, %s" % (buf.raw[:n].count(b"\n"), hashlib.sha256(buf.raw[:n]).hexdigest()))
    finally:
        d.close()


def main():
    lib = os.path.abspath(sys.argv[1])
    if len(sys.argv) > 2:
        return child(lib, sys.argv[2], sys.argv[3])
    with tempfile.TemporaryDirectory() as folder:
        make_streams(folder)
        for name, (_, switches) in CASES.items():
            env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            env.update(switches, DABPHY_DEBUG="1")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), lib, name, folder], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            print("%s%s" % (name, "".join(" %s=%s" % kv for kv in switches.items())))
            for line in r.stderr.splitlines():
                if "decode plan for" in line or "through k_msc_gather + k_viterbi" in line:
                    print("  " + line)
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                sys.stdout.write(r.stderr)
                sys.exit("case %s ended with status %d" % (name, r.returncode))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
