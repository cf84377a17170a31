"""The seven public headers of liblist_hip.so, the ctypes table that binds each, and what the library exports."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# header -> (binding module, its exports table, the prefixes its symbols own; None for list_hip.h, which owns the rest)
SECTIONS = {
    "list_hip.h": ("hip", "EXPORTS", None),
    "list_mesh.h": ("mesh", "MESH_EXPORTS", ("list_mc_", "list_mesh_")),
    "list_eval.h": ("evaluate", "EVAL_EXPORTS", ("list_eval_",)),
    "list_data.h": ("prepare", "DATA_EXPORTS", ("list_data_",)),
    "list_loss.h": ("chamfer", "LOSS_EXPORTS", ("list_chamfer_", "list_loss_")),
    "list_refine.h": ("refine", "REFINE_EXPORTS", ("list_refine_",)),
    "list_voxenc.h": ("voxenc", "VOXENC_EXPORTS", ("list_voxenc_",)),
}


def declared(header):
    """Sorted names of the functions include/<header> declares (comments stripped)."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(list_[a-z0-9_]+)\s*\(", text)))


def exported(lib_path):
    """Every list_* function the built library defines, read with nm."""
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True)
    return set(re.findall(r"\bT (list_\w+)", nm.stdout))
