#!/usr/bin/env python3
"""Write the crystals of CIF files as one shard file (cartnet_amd/shard.py): each asymmetric unit is expanded to the
contents of its unit cell with the file's own symmetry operators, all crystals in one pass on the GPU
(cartnet_amd/symmetry.py), and -- unless ``--unlabeled`` -- the file's ``U_ij`` become the Cartesian targets.

    python tools/cif_to_shard.py DIR/train.cnshard cifs/train/                  # labeled, geometry only
    python tools/cif_to_shard.py DIR/train.cnshard cifs/train/ --radius 5       # with the radius graph, built on the GPU
    python tools/cif_to_shard.py predict.cnshard a.cif b.cif --unlabeled --temperature 150

The reference's filters decide which crystals are used (dataset/extract_csd_data.py:49-56, :95-97: no pressure, no
disorder, a temperature -- ``--temperature K`` fills in a missing one --, labeled: every non-hydrogen atom anisotropic);
``OUT.rejected.txt`` lists the others, one ``name<TAB>reason`` per line.  Crystals are named after their data blocks.  A
directory holding ``train.cnshard``, ``val.cnshard`` and ``test.cnshard`` written this way trains under
``main.py --shard_dir`` as it stands (a geometry-only shard is graphed at load).  Temperatures are stored in Kelvin."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cartnet_amd.cif import load_crystals                                       # noqa: E402


def convert(out_path: str, inputs, labeled: bool = True, temperature=None, radius=None, device: str = "cuda:0") -> dict:
    """Returns ``{"crystals", "atoms", "rows", "rejected", "output"}``; writes ``out_path`` and its ``.rejected.txt``."""
    from cartnet_amd.shard import DeviceShard, write_arrays
    from cartnet_amd.symmetry import expand
    crystals, rejected = load_crystals(inputs, labeled, temperature)
    stem = out_path[:-len(".cnshard")] if out_path.endswith(".cnshard") else out_path
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(stem + ".rejected.txt", "w") as f:
        f.writelines(f"{name}\t{why}\n" for name, why in rejected)
    if not crystals:
        raise SystemExit(f"no usable crystal among the inputs ({len(rejected)} rejected, see {stem}.rejected.txt)")
    arrays, sym = expand(crystals, device, labeled=labeled, temperature=temperature)
    graph = None
    if radius is not None:
        shard = DeviceShard(arrays, device, labeled=labeled, names=sym.names).with_radius_graph(radius)
        arrays = {k: v.cpu().numpy() for k, v in shard.t.items()}
        graph = shard.graph
    write_arrays(out_path, arrays, graph=graph, names=sym.names)
    return {"crystals": len(crystals), "atoms": int(arrays["atom_ptr"][-1]), "rows": int(arrays["y_ptr"][-1]),
            "rejected": len(rejected), "output": out_path}


def main(argv=None) -> dict:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("out", help="the shard file to write (OUT.cnshard); OUT.rejected.txt goes beside it")
    p.add_argument("inputs", nargs="+", help="CIF files, or directories whose *.cif files are read")
    p.add_argument("--unlabeled", action="store_true", help="no targets: crystals to predict ADPs for")
    p.add_argument("--temperature", type=float, default=None, help="Kelvin, for crystals whose file gives no temperature")
    p.add_argument("--radius", type=float, default=None, help="also build the radius graph (uncapped) and record it")
    p.add_argument("--device", type=str, default="cuda:0")
    a = p.parse_args(argv)
    res = convert(a.out, a.inputs, not a.unlabeled, a.temperature, a.radius, a.device)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
