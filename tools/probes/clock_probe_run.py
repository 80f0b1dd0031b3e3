"""Shader clock held inside the persistent GEMM kernel (diagnostic build -DWANQ_CLOCK_PROBE: one workgroup reads clock64 /
wall_clock64 around its main loop; the library prints one [clock] line per launch).
usage: clock_probe_run.py lib_clock.so   (build: hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -shared -DWANQ_CLOCK_PROBE csrc/*.hip)"""
import ctypes, sys, torch
lib = ctypes.CDLL(sys.argv[1])
lib.wanq_gemm_w8a8.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
st = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda").manual_seed(0)
for (M, N, K) in [(32760, 1536, 1536), (32760, 8960, 1536), (32760, 1536, 8960)]:
    a = torch.randint(-127, 128, (M, K), device="cuda", dtype=torch.int8, generator=g)
    w = torch.randint(-127, 128, (N, K), device="cuda", dtype=torch.int8, generator=g)
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    sa = torch.rand(M, device="cuda", generator=g) * 0.01
    asum = a.float().sum(1)
    sw = torch.rand(N, device="cuda", generator=g) * 0.01
    zp = torch.zeros(N, device="cuda")
    print(f"--- gemm {M}x{N}x{K}", flush=True)
    for _ in range(12):
        rc = lib.wanq_gemm_w8a8(a.data_ptr(), w.data_ptr(), out.data_ptr(), 1, sa.data_ptr(), asum.data_ptr(), 2, sw.data_ptr(), None, 2, zp.data_ptr(), 2, None, None, 0, M, N, K, st)
        assert rc == 0, rc
    torch.cuda.synchronize()
