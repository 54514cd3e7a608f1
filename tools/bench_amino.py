"""BASELINE config 5 as amino acids, one rank's share: 12.5 GB of residues (uniform over the 20 letters, generated on
the device with torch), dayhoff, ksize = 27 (9 residues), scaled = 1000, abundance tracking -- in two shapes: 12 500
records of 1 MB, and records of 300 residues.  Writes profiles/r12_bench_amino.json: end-to-end ms, kernel ms
(smh_profile_get "amino_tiled"), windows/s, and the yardstick of the same session: the time per hashed window of
k_protein_fused<9> on the same number of bytes of DNA (the config-5 protein arm, as tools/bench_c5.py runs it; that
kernel hashes two windows per position).  Not part of the test suite.   python tools/bench_amino.py [total_bytes]"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from __graft_entry__ import load_package
pkg = load_package()
L = pkg.lib()
total = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000_000
MAXH = (1 << 64) // 1000
W = 9


def prof(name):
    ms, n = C.c_double(), C.c_uint64()
    L.smh_profile_get(name.encode(), C.byref(ms), C.byref(n))
    return ms.value, n.value


def timed(fn):
    """warm-up on a slice is the caller's; here: one untimed full call, then the timed one with the kernel clock on"""
    fn(); torch.cuda.synchronize()
    L.smh_profile_reset(); L.smh_profile_enable(1)
    t0 = time.perf_counter(); mh = fn(); torch.cuda.synchronize(); dt = time.perf_counter() - t0
    L.smh_profile_enable(0)
    return mh, dt * 1e3


letters = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device="cuda")
buf = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
step = 1 << 28
g = torch.Generator(device="cuda"); g.manual_seed(12)
for lo in range(0, total, step):
    n = min(step, total - lo)
    buf[lo:lo + n] = letters[torch.randint(0, 20, (n,), device="cuda", generator=g)]
torch.cuda.synchronize()

out = {"total_bytes": total, "ksize": 27, "alphabet": "dayhoff", "scaled": 1000, "shapes": {}}
for name, rlen in (("records_1MB", 1_000_000), ("records_300", 300)):
    nrec = total // rlen
    off = np.arange(nrec + 1, dtype=np.uint64) * np.uint64(rlen)
    used = int(off[-1])

    def run():
        mh = pkg.KmerMinHash(0, 27, True, 42, MAXH, True, alphabet="dayhoff")
        mh.add_proteins_dev(buf.data_ptr(), used, off)
        return mh

    mh, ms = timed(run)
    kms, launches = prof("amino_tiled")
    windows = nrec * (rlen - W + 1)
    out["shapes"][name] = {"records": nrec, "end_to_end_ms": ms, "amino_tiled_ms": kms, "launches": launches, "windows": windows,
                           "windows_per_s": windows / (kms / 1e3) if kms else None, "ns_per_window": kms * 1e6 / windows if kms else None,
                           "sketch_hashes": len(mh)}
    print(name, out["shapes"][name], flush=True)

# the yardstick: the translated protein arm on as many bytes of DNA, 1 MB records
assert L.smh_synth_dna_dev(C.c_void_p(buf.data_ptr()), 0, total - total % 32, 5, 0, None) == 0
torch.cuda.synchronize()
rlen = 1_000_000
nrec = (total - total % 32) // rlen
off = np.arange(nrec + 1, dtype=np.uint64) * np.uint64(rlen)


def run_dna():
    mh = pkg.KmerMinHash(0, 27, True, 42, MAXH, True)
    mh.add_sequences_dev(buf.data_ptr(), int(off[-1]), off, True)
    return mh


mh, ms = timed(run_dna)
kms, launches = prof("protein_fused")
windows = sum(2 * max(0, (rlen - f) // 3 - W + 1) for f in range(3)) * nrec
out["protein_fused_yardstick"] = {"records": nrec, "end_to_end_ms": ms, "protein_fused_ms": kms, "launches": launches,
                                  "windows": windows, "ns_per_window": kms * 1e6 / windows if kms else None}
print("protein_fused", out["protein_fused_yardstick"], flush=True)
with open(os.path.join(ROOT, "profiles", "r12_bench_amino.json"), "w") as fh:
    json.dump(out, fh, indent=1)
