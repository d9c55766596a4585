#!/usr/bin/env python
"""Outputs of the five psi calls (cimrgp_psi1, cimrgp_psi2, cimrgp_psi1_grad, cimrgp_psi2_grad, cimrgp_psi2_rows_quad) from
fixed seeds, as .npy files:

    CIMRGP_LIB_PATH=<library A> python tools/psi_ab.py dump out_a
    CIMRGP_LIB_PATH=<library B> python tools/psi_ab.py dump out_b
    python tools/psi_ab.py compare out_a out_b        (host only)

`compare` views every pair of arrays as integers: two builds of the library that keep the launch geometries and the
summation orders give the same bits in every file.  Both dtypes throughout: the shapes of the kernel tests, (130, 70, d)
for every d (two tile rows at edge 64, three at edge 32, a ragged last tile, three slices), every q instance of the
rows call, odd and padded pitches of every matrix operand, bad rows in the first, a middle and the last workgroup of 256
rows, and the shapes whose slices are longer than one 64-row chunk.  An output above 16 MiB is kept as its SHA-256.
Well under a minute.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

DTS = ("f64", "f32")
SHAPES = [(1, 1, 1), (255, 63, 2), (300, 65, 3), (257, 130, 8), (150, 40, 2), (64, 321, 2)] + [(130, 70, d) for d in range(1, 9)]
ELLS = [0.75, 1.25, 1.0, 0.875, 1.5, 1.125, 0.625, 1.0]
SF2 = 1.375
CALLS = ("psi1", "psi2", "psi1_grad", "psi2_grad", "rows")


def dump(out_dir):
    import torch

    import cimrgp_amd
    from cimrgp_amd import device_psi as dp
    dev = cimrgp_amd.device
    dev.require_gpu()
    os.makedirs(out_dir, exist_ok=True)
    tdt = {"f64": torch.float64, "f32": torch.float32}
    count = [0]

    def save(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            a = np.ascontiguousarray(t.detach().cpu().numpy())
            if a.nbytes > (16 << 20):
                a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            np.save(os.path.join(out_dir, "%s.%d.npy" % (name, i)), a)
            count[0] += 1

    def pitch_of(cols, pitch):
        return dev.padded_ld(cols) if pitch == "pad" else cols + 1 + cols % 2          # "odd": the next odd number above cols

    def zeros(rows, cols, dt, pitch):
        """A zeroed (rows x cols) view of a buffer with the given pitch: what a call leaves unwritten compares equal."""
        return torch.zeros((rows, pitch_of(cols, pitch)), dtype=tdt[dt], device="cuda")[:, :cols]

    def mat(a, dt, pitch):
        v = zeros(a.shape[0], a.shape[1], dt, pitch)
        v.copy_(torch.as_tensor(np.ascontiguousarray(a)).to("cuda", tdt[dt]))
        return v

    def vec(a, dt):
        return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", tdt[dt]).contiguous()

    def run(tag, dt, n, m, d, q=2, pitch="pad", bad_rows=(), calls=CALLS):
        g = np.random.default_rng([n, m, d, q])
        mu, z = g.normal(size=(n, d)), 1.5 * g.normal(size=(m, d))
        s = g.uniform(0.0, 0.6, size=(n, d))
        s[::7] = 0.0
        for row, value in bad_rows:
            s[row, (row + 1) % d] = value
        g2 = g.normal(size=(m, m))
        c = g.normal(size=(m, m))
        mu, s, z = vec(mu, dt), vec(s, dt), vec(z, dt)
        ell = torch.as_tensor(np.array(ELLS[:d])).to("cuda")
        name = "%s_%s_%d_%d_%d_%d_%s" % (tag, dt, n, m, d, q, pitch)
        if "psi1" in calls:
            save(name + "_psi1", dp.psi1(mu, s, z, ell, SF2, out=zeros(n, m, dt, pitch)))
        if "psi2" in calls:
            save(name + "_psi2", *dp.psi2(mu, s, z, ell, SF2, out=zeros(m, m, dt, pitch)))
        if "psi1_grad" in calls:
            save(name + "_psi1g", *dp.psi1_grad(mu, s, z, ell, SF2, mat(g.normal(size=(n, m)), dt, pitch)))
        if "psi2_grad" in calls:
            save(name + "_psi2g", *dp.psi2_grad(mu, s, z, ell, SF2, mat(g2 + g2.T, dt, pitch)))
        if "rows" in calls:
            save(name + "_rows", *dp.psi2_rows_quad(mu, s, z, ell, SF2, mat(c + c.T, dt, pitch), mat(g.normal(size=(m, q)), dt, pitch),
                                                    quad=zeros(n, q, dt, pitch)))

    for dt in DTS:
        for n, m, d in SHAPES:
            run("shape", dt, n, m, d)
        for n, m, d in ((130, 70, 3), (255, 63, 2)):
            for q in (1, 3, 4, 5, 8):                                  # 5 runs the Q = 8 instance with zero columns
                run("q", dt, n, m, d, q=q, calls=("rows",))
        for n, m, d in ((255, 63, 2), (130, 70, 5), (64, 321, 2)):
            run("pitch", dt, n, m, d, q=3, pitch="odd")
        # three workgroups of 256 rows in the pass over the rows: a bad row in the first, the middle and the last
        run("bad", dt, 700, 70, 2, bad_rows=((5, -0.25), (300, float("nan")), (699, float("inf"))), calls=("psi2", "psi2_grad", "rows"))
        run("bad", dt, 700, 70, 3, bad_rows=((255, float("inf")), (256, -1.0), (512, float("nan"))), calls=("psi2", "psi2_grad", "rows"))
        # slices longer than one 64-row chunk: 27 slices of 80 rows; one slice of 144 rows over 2080 tiles
        run("chunks", dt, 2113, 4096, 1, calls=("psi1_grad",))
        run("chunks", dt, 130, 4096, 1, calls=("psi2", "psi2_grad", "rows"))
    print("psi_ab: %d arrays written to %s" % (count[0], out_dir))


def compare(dir_a, dir_b):
    names_a, names_b = sorted(os.listdir(dir_a)), sorted(os.listdir(dir_b))
    if names_a != names_b or not names_a:
        print("psi_ab: the two directories do not hold the same files")
        return 1
    differing = []
    for name in names_a:
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        bits = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
        same = a.dtype == b.dtype and a.shape == b.shape
        if not (same and np.array_equal(np.ascontiguousarray(a).view(bits), np.ascontiguousarray(b).view(bits))):
            differing.append(name)
    print("psi_ab: %d arrays compared, %d differ%s"
          % (len(names_a), len(differing), (": " + ", ".join(differing[:20])) if differing else ""))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
