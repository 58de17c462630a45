"""Loader of tests/golden/dpid_vectors.npz (tests/golden/make_dpid_vectors.py: the problems of dp_vectors.npz recorded from the reference's own DP routines at
two pairs of SEPARATE gap-open costs).  Block(b) has the interface of dpvec.Vectors (the checks of test_gpu_dp_forms.py take it as it is) for the cost pair b."""
import json
import os

import numpy as np

import dpvec

HERE = os.path.dirname(os.path.abspath(__file__))


class Block(dpvec.Vectors):
    def __init__(self, b):
        z = np.load(os.path.join(HERE, "golden", "dpid_vectors.npz"))
        self.kind, self.cls, self.init, self.W, self.w_param = z["kind"], z["cls"], z["init"], z["W"], z["w_param"]
        self.qlen, self.tlen, self.view = z["qlen"], z["tlen"], z["view"]
        self.read_off, self.read_codes = z["read_off"], z["read_codes"]
        self.aln, self.cig_off, self.cig = z["aln%d" % b], z["cig_off%d" % b], z["cig%d" % b]
        self.differs, self.redrawn = z["differs%d" % b].astype(bool), z["redrawn"].astype(bool)
        self.I, self.D = (int(x) for x in z["costs"][b])
        self.meta = json.loads(str(z["meta"]))
        self.n = self.kind.size
