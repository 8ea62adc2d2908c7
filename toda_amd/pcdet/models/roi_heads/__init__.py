from .roi_head_template import RoIHeadTemplate
from .second_head import SECONDHead

__all__ = {
    "RoIHeadTemplate": RoIHeadTemplate,
    "SECONDHead": SECONDHead,
}
