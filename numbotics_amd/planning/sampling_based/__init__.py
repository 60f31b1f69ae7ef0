__all__ = ["Connector", "ConnectorParams", "DiscreteConnector", "ContinuousConnector", "StateSpace", "EuclideanSpace", "PlannerParams", "PRM", "PRMStar", "RRT", "RRTStar",
           "Node", "knn_prefix"]

from .connectors import Connector, ConnectorParams, ContinuousConnector, DiscreteConnector
from .roadmap import StateSpace, EuclideanSpace, PlannerParams, PRM, PRMStar, RRT, RRTStar, Node, knn_prefix
