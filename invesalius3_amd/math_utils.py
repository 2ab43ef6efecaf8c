"""``invesalius.math_utils`` -- the host arithmetic of the measures: distance, angle, ellipse area and circumference, polygon
area and perimeter.  Plain Python / numpy with the reference's operation order, so that the numbers a measure stores are
the reference's bit for bit (tests/test_density_host.py compares them with its own output, tests/golden/ref_density.npz).
Nothing here runs on the GPU: a measure has a handful of points."""
from __future__ import annotations

import math

import numpy as np


def calculate_distance(p1, p2) -> float:
    """Euclidean distance of two points of any (equal) dimension: the squares summed in order by ``sum``, then one sqrt."""
    squares = [(b - a) ** 2 for a, b in zip(p1, p2)]
    return math.sqrt(sum(squares))


def calculate_angle(v1, v2) -> float:
    """the angle between two vectors in degrees: acos(dot / (|v1| |v2|))"""
    norms = np.linalg.norm(v1) * np.linalg.norm(v2)
    return math.degrees(math.acos(np.dot(v1, v2) / norms))


def calc_ellipse_area(a: float, b: float) -> float:
    """pi a b, multiplied left to right"""
    return np.pi * a * b


def calc_ellipse_circumference(a: float, b: float) -> float:
    """Ramanujan's first approximation pi (3 (p + q) - sqrt((3 p + q) (p + 3 q))) -- of p = a / 2 and q = b / 2: the reference
    halves the radii it is given before it applies the formula, and so does this."""
    p = a / 2
    q = b / 2
    return np.pi * (3.0 * (p + q) - np.sqrt((3.0 * p + q) * (p + 3.0 * q)))


def calc_polygon_area(points) -> float:
    """the shoelace sum over the closed polygon, (x_prev + x) (y_prev - y) per edge starting with the closing edge, then
    abs(sum / 2)"""
    total = 0.0
    prev = len(points) - 1
    for k in range(len(points)):
        total += (points[prev][0] + points[k][0]) * (points[prev][1] - points[k][1])
        prev = k
    return abs(total / 2.0)


def calc_polygon_perimeter(points) -> float:
    """the edge lengths of the closed polygon summed in order, np.sqrt of (dx^2 + dy^2) each"""
    total = 0.0
    count = len(points)
    for k in range(count):
        xa, ya = points[k]
        xb, yb = points[(k + 1) % count]
        total += np.sqrt((xb - xa) ** 2 + (yb - ya) ** 2)
    return total
