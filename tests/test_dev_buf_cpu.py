"""CPU suite: dev_buf<T> (openair4g_amd/csrc/oai4g_dev_buf.h), the owner of per-configuration device memory.

One stand-alone C++17 program, built with the address and undefined-behaviour sanitizers, includes the header
over host-memory stand-ins for hipMalloc / hipFree / hipMemcpy that count live allocations and can be told to
fail the k-th allocation or copy.  The failure paths of the host layer's uploads and work buffers can only be
exercised here: a real allocation is never made to fail on a device.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openair4g_amd", "csrc")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
static int live = 0, n_alloc = 0, n_copy = 0, n_free = 0;   /* live allocations; calls so far */
static int fail_alloc = 0, fail_copy = 0;                   /* fail the k-th call from now (1 = the next), 0 = none */
static hipError_t hipMalloc(void **p, size_t bytes)
{
  n_alloc++;
  if (fail_alloc && --fail_alloc == 0) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = malloc(bytes ? bytes : 1);
  live++;
  return hipSuccess;
}
static hipError_t hipFree(void *p)
{
  n_free++;
  if (p) live--;
  free(p);
  return hipSuccess;
}
static hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
  n_copy++;
  if (fail_copy && --fail_copy == 0) return hipErrorInvalidValue;
  memcpy(dst, src, bytes);
  return hipSuccess;
}

#include "oai4g_dev_buf.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main()
{
  const std::vector<int> a = {1, 2, 3, 4}, b = {9, 8, 7, 6, 5, 4};
  {
    dev_buf<int> d;
    CHECK(!d && d.get() == nullptr && d.count() == 0);
    CHECK(d.upload(a) == hipSuccess && d && d.count() == 4 && live == 1);
    CHECK(memcmp(d.get(), a.data(), 16) == 0);
    /* a failed upload keeps the old contents: failing allocation, then failing copy */
    const int *old = d.get();
    fail_alloc = 1;
    CHECK(d.upload(b) == hipErrorOutOfMemory);
    CHECK(d.get() == old && d.count() == 4 && live == 1 && memcmp(d.get(), a.data(), 16) == 0);
    fail_copy = 1;
    CHECK(d.upload(b.data(), b.size()) == hipErrorInvalidValue);
    CHECK(d.get() == old && d.count() == 4 && live == 1 && memcmp(d.get(), a.data(), 16) == 0);
    /* a successful one replaces them and frees the old buffer */
    CHECK(d.upload(b) == hipSuccess && d.count() == 6 && live == 1 && memcmp(d.get(), b.data(), 24) == 0);
    /* reserve with a smaller or equal count makes no call at all */
    const int na = n_alloc, nf = n_free, nc = n_copy;
    old = d.get();
    CHECK(d.reserve(3) == hipSuccess && d.reserve(6) == hipSuccess);
    CHECK(n_alloc == na && n_free == nf && n_copy == nc && d.get() == old && d.count() == 6);
    /* a growing one frees first, copies nothing */
    CHECK(d.reserve(100) == hipSuccess && d.count() == 100 && live == 1 && n_free == nf + 1 && n_copy == nc);
    d.get()[99] = 1;
    /* and when it fails the object is empty, not dangling */
    fail_alloc = 1;
    CHECK(d.reserve(1000) == hipErrorOutOfMemory);
    CHECK(!d && d.get() == nullptr && d.count() == 0 && live == 0);
    CHECK(d.reserve(2) == hipSuccess && d.count() == 2 && live == 1);
    d.reset();
    CHECK(!d && d.count() == 0 && live == 0);
    d.reset();
    CHECK(live == 0);
  }
  {
    /* moves leave the source empty and free nothing twice */
    dev_buf<int> s;
    CHECK(s.upload(a) == hipSuccess);
    const int *p = s.get();
    dev_buf<int> t(std::move(s));
    CHECK(!s && s.count() == 0 && t.get() == p && t.count() == 4 && live == 1);
    dev_buf<int> u;
    CHECK(u.upload(b) == hipSuccess && live == 2);
    u = std::move(t);
    CHECK(!t && t.count() == 0 && u.get() == p && u.count() == 4 && live == 1);
    dev_buf<int> &self = u;
    u = std::move(self);
    CHECK(u.get() == p && u.count() == 4 && live == 1);
    std::vector<dev_buf<int>> v(3);
    v[1] = std::move(u);
    v.resize(40);                       /* relocates by move */
    CHECK(v[1].get() == p && live == 1);
  }
  CHECK(live == 0);
  int *kept = nullptr;
  const int nf = n_free;
  {
    /* release() followed by destruction frees nothing */
    dev_buf<int> d;
    CHECK(d.upload(a) == hipSuccess);
    kept = d.release();
    CHECK(kept && !d && d.count() == 0 && live == 1);
  }
  CHECK(n_free == nf && live == 1 && kept[3] == 4);
  hipFree(kept);
  CHECK(live == 0);
  printf("%d failures, %d live\n", failures, live);
  return failures || live ? 1 : 0;
}
"""


def test_dev_buf_under_sanitizers():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "dev_buf_test.cpp"), os.path.join(d, "dev_buf_test")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
        run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failures, 0 live")
