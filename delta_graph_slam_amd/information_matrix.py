"""Edge information matrices from the NN fitness score: the reference's InformationMatrixCalculator over the HIP kernels.

Mirrors /root/reference/src/hdl_graph_slam/information_matrix_calculator.cpp:28-75,110-157 (parameters, calc_information_matrix and
the two building forms) and include/hdl_graph_slam/information_matrix_calculator.hpp:46-54 (weight, b_weight); calc_fitness_score
(:77-108) runs on the device (called per odometry edge and per loop edge, apps/delta_graph_slam_nodelet.cpp:572,820,
each time building a fresh kd-tree on the CPU in the reference).

A tick's edges go through calc_information_matrices: every edge's clouds are DeviceClouds (the loop detector's resident keyframes when
the calculator was given `resident=detector.resident`), the NN indices that are missing are built in one batch and kept in the clouds,
and all edges are walked by one launch (dgs_calc_fitness_score_batch_clouds).

fitness_score_thresh: the reference has two defaults, 0.5 in the constructor (.cpp:38) and 2.5 in the `load` template (.hpp:35).  The
nodelet constructs the calculator from its node handle, so the constructor's 0.5 is mirrored here.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence

import numpy as np

__all__ = ["InformationMatrixCalculator"]
DBL_MAX = 1.7976931348623157e308


class InformationMatrixCalculator:
    def __init__(self, params: Optional[dict] = None, registration=None, device: Optional[int] = None, resident: Optional[Callable] = None):
        pr = dict(params or {})
        self.use_const_inf_matrix = bool(pr.get("use_const_inf_matrix", False))
        self.const_stddev_x = float(pr.get("const_stddev_x", 0.5))
        self.const_stddev_q = float(pr.get("const_stddev_q", 0.1))
        self.var_gain_a = float(pr.get("var_gain_a", 20.0))
        self.min_stddev_x = float(pr.get("min_stddev_x", 0.1))
        self.max_stddev_x = float(pr.get("max_stddev_x", 5.0))
        self.min_stddev_q = float(pr.get("min_stddev_q", 0.05))
        self.max_stddev_q = float(pr.get("max_stddev_q", 0.2))
        self.fitness_score_thresh = float(pr.get("fitness_score_thresh", 0.5))
        # .cpp:40-48
        self.b_var_gain_a = float(pr.get("delta_var_gain_a", 20.0))
        self.b_min_stddev_x = float(pr.get("delta_min_stddev_x", 0.1))
        self.b_max_stddev_x = float(pr.get("delta_max_stddev_x", 5.0))
        self.b_min_stddev_q = float(pr.get("delta_min_stddev_q", 0.05))
        self.b_max_stddev_q = float(pr.get("delta_max_stddev_q", 0.2))
        self.b_avg_fitness_score = float(pr.get("delta_avg_fitness_score", 0.5))
        self.b_importance_ratio_global = float(pr.get("delta_importance_ratio_global", 1.0))
        self.b_importance_ratio_local = float(pr.get("delta_importance_ratio_local", 1.0))
        if registration is None and not self.use_const_inf_matrix:
            from .registration import Registration
            registration = Registration("NDT_OMP", device=device)   # any handle: only its NN machinery is used
        self.registration = registration
        # KeyFrame -> its HBM-resident cloud (LoopDetector.resident): the upload and index made here are the loop detector's next
        self.resident = resident

    @staticmethod
    def weight(a: float, max_x: float, min_y: float, max_y: float, x: float) -> float:
        y = (1.0 - math.exp(-a * x)) / (1.0 - math.exp(-a * max_x))
        return min_y + (max_y - min_y) * y

    @staticmethod
    def b_weight(a: float, avg_x: float, min_y: float, max_y: float, x: float) -> float:
        """.hpp:51-54; exp overflows to inf as std::exp does (inf / inf = NaN there too)."""
        try:
            ex = math.exp(a * (x - avg_x))
        except OverflowError:
            ex = math.inf
        y = ex / (ex + 1.0) if ex != math.inf else math.nan
        return min_y + (max_y - min_y) * y

    # ---- fitness ---------------------------------------------------------------------------------------------------------
    def _cloud(self, c):
        """A KeyFrame becomes its resident cloud (or its array when the calculator was given no `resident`)."""
        from .loop_detector import KeyFrame
        if isinstance(c, KeyFrame):
            return self.resident(c, True) if self.resident is not None else c.cloud
        return c

    def calc_fitness_score(self, cloud1, cloud2, relpose, max_range: float = DBL_MAX) -> float:
        from .registration import DeviceCloud
        cloud1, cloud2 = self._cloud(cloud1), self._cloud(cloud2)
        if isinstance(cloud1, DeviceCloud) or isinstance(cloud2, DeviceCloud):
            return float(self.calc_fitness_scores([(cloud1, cloud2, relpose)], max_range)[0])
        return self.registration.calc_fitness_score(cloud1, cloud2, np.asarray(relpose, np.float64).astype(np.float32), max_range)

    def calc_fitness_scores(self, edges: Sequence, max_range: float = DBL_MAX) -> np.ndarray:
        """calc_fitness_score of every (cloud1, cloud2, relpose) in one device call -> float64 [E]."""
        c1 = [self._cloud(e[0]) for e in edges]
        c2 = [self._cloud(e[1]) for e in edges]
        rel = [np.asarray(e[2], np.float64).astype(np.float32) for e in edges]
        return self.registration.calc_fitness_score_batch(c1, c2, rel, max_range)

    # ---- matrices --------------------------------------------------------------------------------------------------------
    def _const(self) -> np.ndarray:
        inf = np.eye(3)
        inf[:2, :2] /= self.const_stddev_x
        inf[2, 2] /= self.const_stddev_q
        return inf

    def _from_fitness(self, fitness: float) -> np.ndarray:
        """.cpp:63-74: the two weights pass through `float`."""
        w_x = np.float32(self.weight(self.var_gain_a, self.fitness_score_thresh, self.min_stddev_x ** 2, self.max_stddev_x ** 2, fitness))
        w_q = np.float32(self.weight(self.var_gain_a, self.fitness_score_thresh, self.min_stddev_q ** 2, self.max_stddev_q ** 2, fitness))
        inf = np.eye(3)
        inf[:2, :2] /= float(w_x)
        inf[2, 2] /= float(w_q)
        return inf

    def calc_information_matrix(self, cloud1, cloud2, relpose) -> np.ndarray:
        if self.use_const_inf_matrix:
            return self._const()
        return self._from_fitness(self.calc_fitness_score(cloud1, cloud2, relpose))

    def calc_information_matrices(self, edges: Sequence) -> np.ndarray:
        """calc_information_matrix for all edges of a tick -> [E,3,3].  Each edge is (cloud1, cloud2, relpose); a cloud is a DeviceCloud, an
        array / device tensor, or a KeyFrame (see `resident`)."""
        edges = list(edges)
        if self.use_const_inf_matrix:
            return np.stack([self._const() for _ in edges]) if edges else np.zeros((0, 3, 3))
        if not edges:
            return np.zeros((0, 3, 3))
        return np.stack([self._from_fitness(float(f)) for f in self.calc_fitness_scores(edges)])

    def calc_information_matrix_buildings_global(self, fitness_score: float) -> np.ndarray:
        """.cpp:110-132.  The constant matrix is returned undivided, as upstream does."""
        if self.use_const_inf_matrix:
            return self._const()
        return self._from_fitness(float(fitness_score)) / self.b_importance_ratio_global

    def calc_information_matrix_buildings_local(self, result) -> np.ndarray:
        """.cpp:134-157; `result`: a BestFitAlignment (fitness_score.avg_distance, fitness_score.coverage_percentage, isEdgeAligned)."""
        fs = result.fitness_score
        w_x = np.float32(self.b_weight(self.b_var_gain_a, self.b_avg_fitness_score, self.b_min_stddev_x ** 2, self.b_max_stddev_x ** 2, fs.avg_distance))
        w_q = np.float32(self.b_weight(self.b_var_gain_a, self.b_avg_fitness_score, self.b_min_stddev_q ** 2, self.b_max_stddev_q ** 2, fs.avg_distance))
        inf = np.eye(3)
        inf[:2, :2] /= float(w_x)
        inf[2, 2] /= float(w_q)
        if result.isEdgeAligned:
            inf = inf * self.b_importance_ratio_local
        inf = inf * (fs.coverage_percentage / 100.0)
        return inf
