"""Euler angles, rotation matrices and the 12-number goal rows.  NumPy only (tests/far_inputs.py, which oracle/gen_golden.py imports
beside the reference, imports this).  No test in this file."""
import numpy as np


def euler_to_matrix(eul):
    """Rz(yaw) Ry(pitch) Rx(roll) for rows of [roll, pitch, yaw] (scipy's from_euler("xyz"), symbolic_ik.py:420), [n,3,3]."""
    eul = np.asarray(eul, dtype=np.float64)
    sa, sb, sc = (np.sin(eul[:, k]) for k in range(3))
    ca, cb, cc = (np.cos(eul[:, k]) for k in range(3))
    Rm = np.empty((len(eul), 3, 3))
    Rm[:, 0, 0] = cc * cb; Rm[:, 0, 1] = cc * sb * sa - sc * ca; Rm[:, 0, 2] = cc * sb * ca + sc * sa
    Rm[:, 1, 0] = sc * cb; Rm[:, 1, 1] = sc * sb * sa + cc * ca; Rm[:, 1, 2] = sc * sb * ca - cc * sa
    Rm[:, 2, 0] = -sb; Rm[:, 2, 1] = cb * sa; Rm[:, 2, 2] = cb * ca
    return Rm


def m12_to_matrices(M12):
    """[..., 12] rows (R row-major, t) -> [..., 4, 4]."""
    M = np.zeros(M12.shape[:-1] + (4, 4))
    M[..., :3, :3] = M12[..., :9].reshape(M12.shape[:-1] + (3, 3))
    M[..., :3, 3] = M12[..., 9:]
    M[..., 3, 3] = 1.0
    return M


def m12_soa_to_matrices(m12):
    """The device's layout [n_steps, 12, k] -> [n_steps, k, 4, 4]."""
    return m12_to_matrices(np.moveaxis(m12, 1, 2))
