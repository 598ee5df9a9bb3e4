"""Generates tests/golden/channel_ref.json and channel_ref.npz from the reference's own fading channel.

SIMULATION/TOOLS/random_channel.c and multipath_channel.c are compiled unmodified into a temporary directory outside
the repository, with glue of ours: a four-function cblas.h / cblas with plain loops, logRecord and opp_enabled, and
gaussdouble / uniformrandom that return a scripted sequence.  Built without FMA contraction (-ffp-contract=off), so the
convolution's doubles are the separate multiplies and adds the source states.  They run the cases of
tests/channel_cases.py and are removed; nothing compiled from the reference is kept.  Run from the repo root, with the
reference tree at $REF (default: where oracle/Makefile looks for it):

    python tests/golden/gen_channel_ref.py

channel_ref.json (one case per line):
  desc     per descriptor case: nb_taps, channel_length, ricean_factor, aoa, random_aoa, amps, delays, R_sqrt (the
           matrices random_channel reads, R_sqrt[i / 3]: [matrix][row][col][re, im])
  conv     per convolution case and input: channel_length, and per receive antenna the digests of rx_re / rx_im
           [|channel_offset|, length) after multipath_channel with keep_channel = 1
  seconds  per convolution case the reference's single-core run time of one multipath_channel call on the generating
           machine
channel_ref.npz (the bulk, 20 000 doubles, kept out of the text fixture): per descriptor case "<name>/a0", "/ch0",
"/a1", "/ch1", a and ch after a first and a second random_channel call on the scripted draws: a [tap][pair][re, im],
ch [pair][k][re, im].  channel_cases.load_ref() puts the two files together.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import channel_cases as CC  # noqa: E402
from gen_sync_time_ref import FLAGS, PHY, R1, REF  # noqa: E402,F401

CHAN = ["-ffp-contract=off", "-include", PHY + "/TOOLS/time_meas.h"]

CBLAS_H = """
enum { CblasRowMajor = 101, CblasNoTrans = 111 };
void cblas_zgemv(int order, int trans, int M, int N, const void *alpha, const void *A, int lda, const void *X, int incX,
                 const void *beta, void *Y, int incY);
void cblas_zcopy(int N, const void *X, int incX, void *Y, int incY);
void cblas_zscal(int N, const void *alpha, void *X, int incX);
void cblas_zaxpy(int N, const void *alpha, const void *X, int incX, void *Y, int incY);
"""
GLUE = """
#include "cblas.h"
#include "SIMULATION/TOOLS/defs.h"
int opp_enabled = 0;
void logRecord(const char *file, const char *func, int line, int comp, int level, const char *format, ...) {}
typedef struct { double x, y; } cz;
static cz cmul(cz a, cz b) { cz r = {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; return r; }
void cblas_zgemv(int order, int trans, int M, int N, const void *alpha, const void *A, int lda, const void *X, int incX,
                 const void *beta, void *Y, int incY)
{
  const cz *a = A, *x = X, al = *(const cz *)alpha, be = *(const cz *)beta;
  cz *y = Y;
  for (int r = 0; r < M; r++) {
    cz s = {0, 0};
    for (int c = 0; c < N; c++) { cz p = cmul(a[r * lda + c], x[c * incX]); s.x += p.x; s.y += p.y; }
    cz u = cmul(al, s), v = cmul(be, y[r * incY]);
    if (be.x == 0 && be.y == 0) v.x = v.y = 0;
    y[r * incY].x = u.x + v.x;
    y[r * incY].y = u.y + v.y;
  }
}
void cblas_zcopy(int N, const void *X, int incX, void *Y, int incY)
{
  for (int i = 0; i < N; i++) ((cz *)Y)[i * incY] = ((const cz *)X)[i * incX];
}
void cblas_zscal(int N, const void *alpha, void *X, int incX)
{
  for (int i = 0; i < N; i++) ((cz *)X)[i * incX] = cmul(*(const cz *)alpha, ((cz *)X)[i * incX]);
}
void cblas_zaxpy(int N, const void *alpha, const void *X, int incX, void *Y, int incY)
{
  for (int i = 0; i < N; i++) {
    cz p = cmul(*(const cz *)alpha, ((const cz *)X)[i * incX]);
    ((cz *)Y)[i * incY].x += p.x;
    ((cz *)Y)[i * incY].y += p.y;
  }
}
static const double *script;
static int script_n, script_i;
void glue_script(const double *p, int n) { script = p; script_n = n; script_i = 0; }
int glue_script_used(void) { return script_i; }
static double next_draw(void) { if (script_i >= script_n) abort(); return script[script_i++]; }
double gaussdouble(double mean, double variance) { return mean + sqrt(variance) * next_draw(); }
double uniformrandom(void) { return next_draw(); }
void *glue_new(int nb_tx, int nb_rx, int model, double BW, double ff, int offset, double pl)
{
  return new_channel_desc_scm(nb_tx, nb_rx, model, BW, ff, offset, pl);
}
void glue_scalars(channel_desc_t *d, int *iv, double *dv)
{
  iv[0] = d->nb_taps; iv[1] = d->channel_length; iv[2] = d->random_aoa; iv[3] = d->first_run;
  dv[0] = d->ricean_factor; dv[1] = d->aoa;
}
double *glue_amps(channel_desc_t *d) { return d->amps; }
double *glue_delays(channel_desc_t *d) { return d->delays; }
double *glue_rsqrt(channel_desc_t *d, int i) { return (double *)d->R_sqrt[i]; }
double *glue_a(channel_desc_t *d, int i) { return (double *)d->a[i]; }
double *glue_ch(channel_desc_t *d, int p) { return (double *)d->ch[p]; }
int glue_random(channel_desc_t *d) { return random_channel(d, 0); }
void glue_multipath(channel_desc_t *d, double **tr, double **ti, double **rr, double **ri, unsigned length)
{
  multipath_channel(d, tr, ti, rr, ri, length, 1);
}
"""


def build(tmp):
    open(os.path.join(tmp, "cblas.h"), "w").write(CBLAS_H)
    glue = os.path.join(tmp, "channel_glue.c")
    open(glue, "w").write(GLUE)
    flags = ["-I", tmp] + FLAGS + CHAN + ["-include", "math.h"]
    objs = []
    for src in (R1 + "/SIMULATION/TOOLS/random_channel.c", R1 + "/SIMULATION/TOOLS/multipath_channel.c", glue):
        obj = os.path.join(tmp, os.path.basename(src) + ".o")
        subprocess.run(["gcc"] + flags + ["-c", src, "-o", obj], check=True)
        objs.append(obj)
    so = os.path.join(tmp, "libref_channel.so")
    subprocess.run(["gcc", "-shared", "-Wl,-Bsymbolic", "-o", so] + objs + ["-lm"], check=True)
    L = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    L.glue_new.restype = ctypes.c_void_p
    L.glue_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                           ctypes.c_double]
    L.glue_scalars.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), dp]
    L.glue_script.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for f in (L.glue_amps, L.glue_delays):
        f.restype, f.argtypes = dp, [ctypes.c_void_p]
    for f in (L.glue_rsqrt, L.glue_a, L.glue_ch):
        f.restype, f.argtypes = dp, [ctypes.c_void_p, ctypes.c_int]
    L.glue_random.argtypes = [ctypes.c_void_p]
    L.glue_multipath.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_void_p)] * 4 + [ctypes.c_uint]
    return L


def scalars(L, d):
    iv, dv = (ctypes.c_int * 4)(), (ctypes.c_double * 2)()
    L.glue_scalars(d, iv, dv)
    return list(iv), list(dv)


def arr(p, shape):
    return np.ctypeslib.as_array(p, shape).copy()


def desc_case(L, name, arrays):
    model, nt, nr, bw, ff = CC.DESC[name]
    d = L.glue_new(nt, nr, CC.MODELS[model], bw, ff, 0, 0.0)
    assert d, name
    (ntap, clen, raoa, first), (rf, aoa) = scalars(L, d)
    n = nt * nr
    assert first == 1
    row = {"nb_taps": ntap, "channel_length": clen, "ricean_factor": rf, "aoa": aoa, "random_aoa": raoa,
           "amps": arr(L.glue_amps(d), (ntap,)).tolist(), "delays": arr(L.glue_delays(d), (ntap,)).tolist(),
           "R_sqrt": [arr(L.glue_rsqrt(d, i), (n, n, 2)).tolist() for i in range((ntap - 1) // 3 + 1)]}
    count = CC.n_draws(ntap, nt, nr, rf, raoa)
    for call in (0, 1):
        seq = CC.draws(name, call, count, n if count > 2 * ntap * n else 0)
        L.glue_script(seq.ctypes.data, len(seq))
        assert L.glue_random(d) == 0 and L.glue_script_used() == count, name
        arrays[f"{name}/a{call}"] = np.stack([arr(L.glue_a(d, i), (n, 2)) for i in range(ntap)])
        arrays[f"{name}/ch{call}"] = np.stack([arr(L.glue_ch(d, p), (clen, 2)) for p in range(n)])
    return row


def conv_case(L, name):
    model, nt, nr, bw, off, length = CC.CONV[name]
    d = L.glue_new(nt, nr, CC.MODELS[model], bw, 0.0, off, 0.0)
    clen = scalars(L, d)[0][1]
    ch = CC.conv_taps(name, clen)
    for p in range(nt * nr):
        np.ctypeslib.as_array(L.glue_ch(d, p), (clen, 2))[:] = np.stack([ch[p].real, ch[p].imag], axis=1)
    out, best = {"channel_length": clen}, None
    dd = abs(off)
    for kind in CC.CONV_INPUTS:
        x = CC.conv_input(name, kind, clen).astype(np.float64)
        tr = [np.ascontiguousarray(x[j, :, 0]) for j in range(nt)]
        ti = [np.ascontiguousarray(x[j, :, 1]) for j in range(nt)]
        rr = [np.full(length, np.nan) for _ in range(nr)]
        ri = [np.full(length, np.nan) for _ in range(nr)]
        pp = [(ctypes.c_void_p * len(v))(*[a.ctypes.data for a in v]) for v in (tr, ti, rr, ri)]
        t0 = time.perf_counter()
        L.glue_multipath(d, *pp, length)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        assert all(np.isnan(r[:dd]).all() and not np.isnan(r[dd:]).any() for r in rr + ri)
        out[kind] = [[CC.digest(rr[a][dd:]), CC.digest(ri[a][dd:])] for a in range(nr)]
    return out, round(best, 4)


def main():
    out, arrays = {"seed": CC.SEED, "desc": {}, "conv": {}, "seconds": {}}, {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for name in CC.DESC:
            out["desc"][name] = desc_case(L, name, arrays)
        for name in CC.CONV:
            out["conv"][name], out["seconds"][name] = conv_case(L, name)
        del L
    np.savez_compressed(os.path.join(HERE, "channel_ref.npz"), **arrays)
    with open(os.path.join(HERE, "channel_ref.json"), "w") as f:            # one case per line
        f.write('{"seed": %d, "seconds": %s,\n' % (out["seed"], json.dumps(out["seconds"], sort_keys=True)))
        for part in ("desc", "conv"):
            rows = ['"%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in sorted(out[part].items())]
            f.write('"%s": {\n%s\n}%s\n' % (part, ",\n".join(rows), "," if part == "desc" else "}"))


if __name__ == "__main__":
    main()
