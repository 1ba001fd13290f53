"""Worker of tests/test_host_options.py: runs inside a python started with LD_PRELOAD=libasan.so and loads the
AddressSanitizer build of the host-only code (`build.sh --host-asan`), which holds the option table of csrc/options.cpp.
Reads the environment into a fresh option set as lpgp_init does, applies the operations of argv[2] (JSON list of
["get", key] / ["set", key, value]) and prints one JSON object: {"rows": {key: value of every row after the environment},
"ops": [[rc, value or error message], ...]} ("set" answers with the value read back after it)."""
import ctypes as C
import json
import sys

lib = C.CDLL(sys.argv[1])
lib.lpgp_host_options_from_env.restype = None
lib.lpgp_host_options_get.restype = C.c_int
lib.lpgp_host_options_get.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
lib.lpgp_host_options_set.restype = C.c_int
lib.lpgp_host_options_set.argtypes = [C.c_char_p, C.c_int64]
lib.lpgp_host_options_count.restype = C.c_int
lib.lpgp_host_options_name.restype = C.c_char_p
lib.lpgp_host_options_name.argtypes = [C.c_int]
lib.lpgp_host_last_error.restype = C.c_char_p


def get(key):
    v = C.c_int64()
    rc = lib.lpgp_host_options_get(key.encode(), C.byref(v))
    return [rc, v.value if rc == 0 else lib.lpgp_host_last_error().decode()]


lib.lpgp_host_options_from_env()
names = [lib.lpgp_host_options_name(i).decode() for i in range(lib.lpgp_host_options_count())]
assert lib.lpgp_host_options_name(len(names)) is None and lib.lpgp_host_options_name(-1) is None
assert len(set(names)) == len(names), "duplicate option keys"
rows = {k: get(k)[1] for k in names}
ops = []
for op in json.loads(sys.argv[2]) if len(sys.argv) > 2 else []:
    if op[0] == "get":
        ops.append(get(op[1]))
    else:
        rc = lib.lpgp_host_options_set(op[1].encode(), op[2])
        ops.append([rc, get(op[1])[1] if rc == 0 else lib.lpgp_host_last_error().decode()])
print(json.dumps({"rows": rows, "ops": ops}))
