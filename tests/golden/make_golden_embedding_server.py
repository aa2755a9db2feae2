"""Generates reference_embedding_server.json: what tests/test_embedding_server.py checks the embedding server against.

Needs a checkout of the reference LEANN repository (and the protobuf runtime):
    python tests/golden/make_golden_embedding_server.py <LEANN checkout>
Two records, both data:
  * "flags": every parser.add_argument(...) call of the two stock embedding servers
    (leann_backend_hnsw/hnsw_embedding_server.py, leann_backend_diskann/diskann_embedding_server.py), read with ``ast``:
    {flag: {"default", "choices", "type"}} per flavour;
  * "protobuf": the bytes the reference's generated embedding_pb2 serialises for the messages the test builds, as hex.
"""
import ast
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SERVERS = {"hnsw": "packages/leann-backend-hnsw/leann_backend_hnsw/hnsw_embedding_server.py",
           "diskann": "packages/leann-backend-diskann/leann_backend_diskann/diskann_embedding_server.py"}
PB2 = "packages/leann-backend-diskann/leann_backend_diskann/embedding_pb2.py"
REQUEST_IDS = [5, 70000, 3, 2**32 - 1]
RESPONSE = {"embeddings_data_f32": [float(v) for v in range(8)], "dimensions": [2, 4], "missing_ids": [9]}


def server_flags(path: Path) -> dict:
    flags = {}
    for node in ast.walk(ast.parse(path.read_text())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            name = ast.literal_eval(node.args[0])
            kw = {k.arg: k.value for k in node.keywords}
            flags[name] = {"default": ast.literal_eval(kw["default"]) if "default" in kw else None,
                           "choices": ast.literal_eval(kw["choices"]) if "choices" in kw else None,
                           "type": kw["type"].id if "type" in kw else None}
    return flags


def main():
    ref = Path(sys.argv[1])
    spec = importlib.util.spec_from_file_location("ref_embedding_pb2", ref / PB2)
    pb2 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pb2)
    req = pb2.NodeEmbeddingRequest()
    req.node_ids.extend(REQUEST_IDS)
    resp = pb2.NodeEmbeddingResponse(embeddings_data=np.array(RESPONSE["embeddings_data_f32"], np.float32).tobytes(), dimensions=RESPONSE["dimensions"],
                                     missing_ids=RESPONSE["missing_ids"])
    out = {"flags": {k: server_flags(ref / v) for k, v in SERVERS.items()},
           "protobuf": {"request": {"node_ids": REQUEST_IDS, "bytes_hex": req.SerializeToString().hex()},
                        "response": dict(RESPONSE, bytes_hex=resp.SerializeToString().hex())}}
    (HERE / "reference_embedding_server.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
