# The host JPEG stage of two builds of libroma_hip.so side by side, on the CPU (no GPU is touched): byte identity of info / coef / qt on the
# bundled photographs and every stream of tests/test_jpeg.py's _synthetic_jpegs(), then the time of roma_jpeg_entropy_decode on the four
# photographs and prog_photo, the two libraries alternating, REPS repetitions of CALLS calls each.
#   python tools/jpeg_host_compare.py OTHER/libroma_hip.so [--dump DIR]
# --dump DIR also writes the synthetic streams and the small ones of the mutation sweep as files, for roma_amd/csrc/jpeg_host_check.
import ctypes, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roma_amd import _lib
from tests import test_jpeg as T

REPS, CALLS = 7, 20


def load(path):
    lib = ctypes.CDLL(path)
    lib.roma_jpeg_info.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    lib.roma_jpeg_entropy_decode.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def decode(lib, data):
    buf, info = np.frombuffer(data, dtype=np.uint8), np.zeros(8, np.int32)
    assert lib.roma_jpeg_info(buf.ctypes.data, len(data), info.ctypes.data) == 0
    coef = np.full((int(info[4]) * int(info[5]) + 2 * int(info[6]) * int(info[7]), 64), -1, np.int16)
    qt = np.full((3, 64), 0xFFFF, np.uint16)
    assert lib.roma_jpeg_entropy_decode(buf.ctypes.data, len(data), coef.ctypes.data, qt.ctypes.data) == 0
    return info, coef, qt


def seconds_per_call(lib, data, coef, qt):
    buf = np.frombuffer(data, dtype=np.uint8)
    t0 = time.perf_counter()
    for _ in range(CALLS):
        lib.roma_jpeg_entropy_decode(buf.ctypes.data, len(data), coef.ctypes.data, qt.ctypes.data)
    return (time.perf_counter() - t0) / CALLS


other, this = load(sys.argv[1]), load(_lib.LIB_PATH)
streams = {os.path.basename(f): open(f, "rb").read() for f in T.ASSETS}
photos = list(streams)
streams.update(T._synthetic_jpegs())
if "--dump" in sys.argv:
    d = sys.argv[sys.argv.index("--dump") + 1]
    os.makedirs(d, exist_ok=True)
    for name, data in {**T._synthetic_jpegs(), **T._small_streams()}.items():
        open(os.path.join(d, name + ".jpg"), "wb").write(data)
same = [all(np.array_equal(a, b) for a, b in zip(decode(other, data), decode(this, data))) for data in streams.values()]
print(f"byte identity of info, coef, qt: {sum(same)} of {len(streams)} streams identical ({', '.join(streams)})")
print(f"roma_jpeg_entropy_decode, ms per call: median of {REPS} repetitions of {CALLS} calls, spread = (max - min) / median, best = the fastest repetition"
      f" (what a shared host disturbs least); other = {sys.argv[1]}")
ok = all(same)
for name in photos + ["prog_photo"]:
    data = streams[name]
    _, coef, qt = decode(this, data)
    t = {"other": [], "this": []}
    for lib in (other, this):
        seconds_per_call(lib, data, coef, qt)                       # warm-up
    for _ in range(REPS):
        t["other"].append(seconds_per_call(other, data, coef, qt))
        t["this"].append(seconds_per_call(this, data, coef, qt))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    within = med["this"] <= med["other"] * (1 + spread["other"])
    ok &= within
    print(f"{name:22s} other {med['other'] * 1e3:7.3f} (spread {spread['other'] * 100:4.1f} %)   this {med['this'] * 1e3:7.3f} (spread {spread['this'] * 100:4.1f} %)"
          f"   this / other {med['this'] / med['other']:.3f}   {'within' if within else 'OUTSIDE'} the other's spread"
          f"   best {min(t['other']) * 1e3:7.3f} / {min(t['this']) * 1e3:7.3f} = {min(t['this']) / min(t['other']):.3f}")
sys.exit(0 if ok else 1)
