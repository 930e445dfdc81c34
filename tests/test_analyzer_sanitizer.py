"""AddressSanitizer + UndefinedBehaviorSanitizer run of the native analyzer (host code of the C-ABI
library).  csrc/analyzer.cpp is compiled with `g++ -fsanitize=address,undefined
-fno-sanitize-recover=all` together with a small driver (tests/native/analyzer_sanitizer_main.cpp)
(the sanitizer runtimes linked statically: the child runs in the environment as it is) and run, as a
child process, over
  * the fuzz corpus of tests/test_tokenizer.py plus the analyzer's edge texts, pre-normalised exactly
    as the product does (lexical.native_input), where the output must equal the product build's, and
  * raw byte strings that are NOT valid UTF-8 -- the product never sends those, a C caller of the ABI
    might: memory-safe, every id in range.
A sanitizer report aborts the child (non-zero exit)."""
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from rag_fin_amd import lexical
from test_analyzer_native_cpu import MORE_EDGE
from test_tokenizer import EDGE, _texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("san") / "analyzer_san"
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "rag_fin_amd", "csrc", "analyzer.cpp"),
           os.path.join(ROOT, "tests", "native", "analyzer_sanitizer_main.cpp"), "-lpthread", "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out)


def _run(driver, tmp_path, blob, offsets, threads):
    punct = lexical._native_tables()[1]    # what the product passes to rf_analyze
    n = len(offsets) - 1
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<q", len(punct)) + punct.tobytes() + struct.pack("<q", n) +
                np.ascontiguousarray(offsets, dtype=np.int64).tobytes() + blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([driver, str(inp), str(threads), str(outp)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stderr[-4000:]}"
    raw = open(outp, "rb").read()
    sizes = np.frombuffer(raw, dtype=np.int64, count=4)
    n_tok, n_terms, vb = int(sizes[1]), int(sizes[2]), int(sizes[3])
    at = 32
    vocab_blob = raw[at:at + vb]
    at += vb
    vocab_off = np.frombuffer(raw, dtype=np.int64, count=n_terms + 1, offset=at)
    at += 8 * (n_terms + 1)
    tok = np.frombuffer(raw, dtype=np.int32, count=n_tok, offset=at)
    at += 4 * n_tok
    dl = np.frombuffer(raw, dtype=np.int64, count=n, offset=at)
    assert at + 8 * n == len(raw) and int(sizes[0]) == n
    return vocab_blob, vocab_off, tok, dl


@pytest.mark.parametrize("threads", [1, 4])
def test_fuzz_corpus_under_asan_ubsan_matches_the_product_build(driver, tmp_path, threads):
    texts = _texts()[1] + MORE_EDGE
    blob, offsets = lexical.native_input(texts)
    vocab_blob, vocab_off, tok, dl = _run(driver, tmp_path, blob, offsets, threads)
    vocab, want_tok, want_dl = lexical.analyze_native(texts)      # the product build of the same source
    assert vocab_blob.decode("utf-8").split("\n")[:-1] == vocab
    assert [vocab_blob[a:b - 1].decode("utf-8") for a, b in zip(vocab_off[:-1].tolist(), vocab_off[1:].tolist())] == vocab
    assert np.array_equal(tok, want_tok) and np.array_equal(dl, want_dl)


def test_malformed_utf8_is_memory_safe(driver, tmp_path):
    rng = random.Random(5)
    blobs = [b"", b"\x80", b"\xc3", b"abc\xe2\x82", b"\xf0\x9f\x98", b"\xff\xfe\xfd", b"a\x00b\x00", b"\xed\xa0\x80",
             b"\xc0\xaf", b"\xf8\x88\x80\x80\x80", b"x" * 5000, b"\xe2" * 300, "é".encode() * 200 + b"\xc3",
             b"\xe2\x80 \x94", b"a\xe2\x80", b"\xe2\x80\x94"[:2] + b"!", b"\xf0\x9f"]
    blobs += [bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 400))) for _ in range(800)]
    blobs += [t.encode("utf-8", "surrogatepass")[:-1] for t in EDGE + MORE_EDGE if t]   # every edge case cut mid-sequence
    offsets = np.zeros(len(blobs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in blobs], out=offsets[1:])
    vocab_blob, vocab_off, tok, dl = _run(driver, tmp_path, b"".join(blobs), offsets, 4)
    n_terms = vocab_off.size - 1
    assert tok.size == int(dl.sum()) and dl.min() >= 0
    assert tok.size == 0 or (tok.min() >= 0 and tok.max() < n_terms)
    terms = [vocab_blob[a:b - 1] for a, b in zip(vocab_off[:-1].tolist(), vocab_off[1:].tolist())]
    assert terms == sorted(set(terms)) and all(t and b"\n" not in t and b" " not in t for t in terms)
