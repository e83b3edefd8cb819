"""Phase timing of the one-launch MinMax encode (minmax_resident.hip) per
kernel configuration, from the kernel's own wall_clock64 stamps
(bagua_minmax_u8_resident_trace): pass 1, exchange, pass 2, per workgroup.
Stamp 0 is kernel entry (before the ticket is drawn), so pass 1 includes the ticket.

  python tools/resident_trace.py [--elements N] [--cfgs 0,1,2]

Prints one JSON line per configuration (medians over workgroups and runs, us).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "bagua-core_amd"))

from bagua_core import _native as N  # noqa: E402

K = N.K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1 << 26)
    ap.add_argument("--cfgs", default="0,1,2,3,4,5")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--decode", action="store_true", help="run the decode between encodes (bench step)")
    ap.add_argument("--dump", default="", help="also save the raw stamps (runs x workgroups x 8, us) to this .npy")
    a = ap.parse_args()
    n = a.elements
    dev = torch.device("cuda", 0)
    x = torch.randn(n, device=dev) * 1e-3
    y = torch.empty_like(x)
    S = K.bagua_minmax_u8_compressed_bytes(0, n, 1)
    comp = torch.empty(S, dtype=torch.uint8, device=dev)
    wsb = K.bagua_minmax_u8_workspace_bytes(n, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tr = torch.zeros(8 * cus, dtype=torch.int64, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    khz = 100000  # wall_clock64: 100 MHz on MI300-class parts (hipDeviceAttributeWallClockRate)
    for cfg in [int(c) for c in a.cfgs.split(",")]:
        os.environ["BAGUA_RESIDENT_CFG"] = str(cfg)
        assert K.bagua_minmax_u8_resident_path(0, x.data_ptr(), n, n, 1, comp.data_ptr(), S, -1, sp) == 1
        rows = []
        for r in range(a.runs + 2):
            K.bagua_minmax_u8_resident_trace(tr.data_ptr() if r >= 2 else None)
            N.check(K.bagua_minmax_u8_compress(0, x.data_ptr(), n, n, 1, comp.data_ptr(), S, ws.data_ptr(), wsb, -1,
                                               sp), "compress")
            K.bagua_minmax_u8_resident_trace(None)
            if a.decode:
                N.check(K.bagua_minmax_u8_decompress(0, comp.data_ptr(), S, n, 1, y.data_ptr(), sp), "decompress")
            if r >= 2:
                torch.cuda.synchronize()
                t = tr.cpu().numpy().reshape(cus, 8).astype(np.float64) * (1e3 / khz)  # us
                t -= t[:, 0].min()
                rows.append(t)
        t = np.stack(rows)  # runs x wg x 8
        if a.dump:
            np.save(a.dump.replace(".npy", f"_cfg{cfg}.npy"), t)
        geo = [ctypes.c_int(0) for _ in range(5)]
        N.check(K.bagua_minmax_u8_resident_cfg_geometry(cfg, *[ctypes.byref(g) for g in geo]), "cfg geometry")
        stack = geo[4].value != 0
        order, rl = ctypes.c_int(0), ctypes.c_int(0)
        N.check(K.bagua_minmax_u8_resident_cfg_order(cfg, ctypes.byref(order), ctypes.byref(rl)), "cfg order")
        window = order.value == 2
        # stack-order rows run pass 2 as held rows (stamp 6), parked rows (stamp 7), streamed part (end);
        # window-order rows as late rows (stamp 6), streamed part (stamp 4), parked rows (stamp 5), early rows
        if window:
            p2 = {"pass2_late_us": t[:, :, 6] - t[:, :, 2], "pass2_stream_us": t[:, :, 4] - t[:, :, 6],
                  "pass2_lds_us": t[:, :, 5] - t[:, :, 4], "pass2_regs_us": t[:, :, 3] - t[:, :, 5]}
        elif stack:
            p2 = {"pass2_regs_us": t[:, :, 6] - t[:, :, 2], "pass2_lds_us": t[:, :, 7] - t[:, :, 6],
                  "pass2_stream_us": t[:, :, 3] - t[:, :, 7]}
        else:
            p2 = {"pass2_stream_us": t[:, :, 4] - t[:, :, 2], "pass2_lds_us": t[:, :, 5] - t[:, :, 4],
                  "pass2_regs_us": t[:, :, 3] - t[:, :, 5]}
        rows_total = n * 4 // 16 // cus // geo[0].value  # rows per slice (f32)
        reread_mb = max(0, rows_total - geo[1].value - geo[2].value - rl.value) * geo[0].value * 16 * cus / 1e6
        out = {
            "cfg": cfg,
            "order": "window" if window else ("stack" if stack else "stream-first"),
            "r": geo[1].value, "h": geo[2].value, "rl": rl.value, "sb": geo[3].value,
            "reread_mb": round(reread_mb, 1),
            "start_spread_us": float(np.median(t[:, :, 0].max(axis=1))),
            "pass1_us_median_wg": float(np.median(t[:, :, 1] - t[:, :, 0])),
            "pass1_end_max_us": float(np.median(t[:, :, 1].max(axis=1))),
            "exchange_us_median_wg": float(np.median(t[:, :, 2] - t[:, :, 1])),
            "exchange_end_max_us": float(np.median(t[:, :, 2].max(axis=1))),
            # from the last workgroup's publish to the last workgroup's leaving the exchange
            "exchange_after_last_pass1_us": float(np.median(t[:, :, 2].max(axis=1) - t[:, :, 1].max(axis=1))),
            "pass2_us_median_wg": float(np.median(t[:, :, 3] - t[:, :, 2])),
            **{k: float(np.median(v)) for k, v in p2.items()},
            "end_max_us": float(np.median(t[:, :, 3].max(axis=1))),
        }
        if reread_mb > 0:
            out["pass2_stream_us_per_100mb"] = round(out["pass2_stream_us"] / reread_mb * 100, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
